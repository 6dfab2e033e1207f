"""CPU-side gate on the kernel of the timetable look-ups (pathplanning_amd/csrc/pp_timetable.hpp): k_timetable_tickets is in the built gfx950 code
object as one wave of 64 lanes (tools/kernel_resources.py reads the figures out of libpphip.so; no GPU needed).

The issue's target was no scratch and no spills.  The build does not reach it: the kernel calls the path readers k_trajectory_tickets calls
(load_edge / PostEdge of pp_postprocess.hpp), whose record arrays live in a private segment of 168 B per lane in both kernels, and no vector register is
spilled.  So, as the issue provides for that case, this file asserts the built figures as upper bounds and the presence of the empty "timetable"
dispatch in warm_up_held_kernels, where the queue allocates that scratch and a failure is an error code; DESIGN.md 4.10 records the same figures."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = "k_timetable_tickets"
VGPRS, SCRATCH = 163, 168  # the figures of the build DESIGN.md 4.10 records


def test_the_kernel_is_built_as_one_wave_within_the_recorded_figures_and_warmed_up():
    from pathplanning_amd import build
    import kernel_resources
    res = {k["kernel"]: k for k in kernel_resources.resources(build.build(verbose=False))}
    assert KERNEL in res, sorted(res)
    k = res[KERNEL]
    print(KERNEL, k)
    src = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_planner.hip")).read()
    reserve = int(re.search(r"constexpr size_t kMaxPrivateBytes = (\d+);", src).group(1))
    assert k["max_flat_workgroup_size"] == 64, k
    assert k["vgpr_spill"] == 0 and k["vgpr"] <= VGPRS, k
    assert k["scratch_bytes_per_lane"] <= SCRATCH <= reserve, k
    assert k["scratch_bytes_per_lane"] <= res["k_trajectory_tickets"]["scratch_bytes_per_lane"]  # no more than the kernel whose readers it shares
    assert k["lds_bytes"] == 0, k  # (its LDS is dynamic: 16 B per path-capacity entry, as the trajectory kernel's)
    warm = src[src.index("hipError_t warm_up_held_kernels"):src.index("int warm_up_kernels")]
    assert 'ok("timetable", launch_timetable(s, p->args' in warm  # (its scratch is allocated at creation)
    assert "trajectory_lds_bytes(args.maxPath)" in src[src.index("hipError_t launch_timetable"):src.index("hipError_t warm_up_held_kernels")]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert KERNEL in design and "%d VGPRs" % VGPRS in design and "%d B" % SCRATCH in design
