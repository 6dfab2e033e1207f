"""CPU-side gate on the kernel of the retime call (pathplanning_amd/csrc/pp_retime.hpp): k_retime_tickets is in the built gfx950 code object as one
wave of 64 lanes, with no scratch and no spilled register (tools/kernel_resources.py reads the figures out of libpphip.so; no GPU needed).  Its LDS
is dynamic -- 8 bytes per hold of the plan with the most holds, at most 8 KiB -- so the code object shows none; having no private segment, it needs
no dispatch in warm_up_held_kernels."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNEL = "k_retime_tickets"


def test_the_kernel_is_built_as_one_wave_without_scratch():
    from pathplanning_amd import build
    import kernel_resources
    res = {k["kernel"]: k for k in kernel_resources.resources(build.build(verbose=False))}
    assert KERNEL in res, sorted(res)
    k = res[KERNEL]
    print(KERNEL, k)
    assert k["max_flat_workgroup_size"] == 64, k
    assert k["scratch_bytes_per_lane"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
    assert k["vgpr"] <= 64, k  # (nothing here needs registers: eight waves per SIMD)
    assert k["lds_bytes"] == 0, k
    src = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_planner.hip")).read()
    launch = src[src.index("hipError_t launch_retime"):src.index("hipError_t launch_wait_places")]
    assert "dim3(kRetimeLanes)" in launch and "retime_lds_bytes(most)" in launch
    kernel = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_retime.hpp")).read()
    assert re.search(r"constexpr int kRetimeLanes = 64;", kernel) and "(size_t)most * 8" in kernel
    rule = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_retime_rule.hpp")).read()
    assert re.search(r"constexpr int kMaxHolds = 1 << 10;", rule)  # 8 KiB of LDS at the most
