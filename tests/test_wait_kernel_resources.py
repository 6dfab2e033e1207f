"""CPU-side gate on the two kernels of a call with waits at stops (pathplanning_amd/csrc/pp_waits.hpp), each in its two forms (k_wait_places<kFixed>,
k_wait_level<kHeading>): they are in the built gfx950 code object as one wave of 64 lanes each (tools/kernel_resources.py reads the figures out of libpphip.so; no GPU needed).  k_wait_level spills no vector register and
takes neither scratch nor LDS.  k_wait_places calls the path readers k_timetable_tickets calls (load_edge / PostEdge of pp_postprocess.hpp), whose
record arrays live in a private segment of 168 B per lane; it spills no vector register, stays within kMaxPrivateBytes and has an empty dispatch in
warm_up_held_kernels, where the queue allocates that scratch and a failure is an error code.  The built figures DESIGN.md 4.10 records are upper
bounds."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# the figures of the build DESIGN.md 4.10 records, the larger of a kernel's two forms (k_wait_places<kFixed>, k_wait_level<kHeading>)
RECORDED = {"k_wait_places": dict(vgpr=145, scratch=168), "k_wait_level": dict(vgpr=86, scratch=0)}


def test_the_two_kernels_are_built_within_the_recorded_figures_and_warmed_up():
    from pathplanning_amd import build
    import kernel_resources
    res = {k["kernel"]: k for k in kernel_resources.resources(build.build(verbose=False))}
    src = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_planner.hip")).read()
    reserve = int(re.search(r"constexpr size_t kMaxPrivateBytes = (\d+);", src).group(1))
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for name, recorded in RECORDED.items():
        forms = [k for kernel, k in res.items() if kernel.split("<")[0] == name]
        assert len(forms) == 2, sorted(res)
        for k in forms:
            print(name, k)
            assert k["max_flat_workgroup_size"] == 64, k
            assert k["vgpr_spill"] == 0 and k["vgpr"] <= recorded["vgpr"], k
            assert k["scratch_bytes_per_lane"] <= recorded["scratch"] <= reserve, k
            assert k["lds_bytes"] == 0, k  # (k_wait_places' LDS is dynamic: 16 B per path-capacity entry, as the trajectory kernel's)
        assert name in design and "%d VGPRs" % recorded["vgpr"] in design
    warm = src[src.index("hipError_t warm_up_held_kernels"):src.index("int warm_up_kernels")]
    assert warm.count('ok("wait places", launch_wait_places(s, p->args') == 2 and 'ok("wait levels", launch_wait_level(s, ' in warm  # (both forms with a private segment)
    assert "trajectory_lds_bytes(args.maxPath)" in src[src.index("hipError_t launch_wait_places"):src.index("hipError_t launch_wait_level")]

