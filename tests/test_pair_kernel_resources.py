"""CPU-side gate on the kernels of the space-time broad phase (pathplanning_amd/csrc/pp_pairs.hpp): they are in the built gfx950 code object, take no
scratch and spill nothing (tools/kernel_resources.py reads the figures out of libpphip.so; no GPU needed).  k_box_pairs is compiled twice, to count and
to fill.  None of them has a private segment, so none needs a line in warm_up_held_kernels."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("k_plan_boxes", "k_box_pairs<false>", "k_box_pairs<true>", "k_pair_offsets")


def test_the_three_kernels_are_built_without_scratch_or_spills():
    from pathplanning_amd import build
    import kernel_resources
    res = {k["kernel"]: k for k in kernel_resources.resources(build.build(verbose=False))}
    for name in KERNELS:
        assert name in res, (name, sorted(res))
        k = res[name]
        print(name, k)
        assert k["scratch_bytes_per_lane"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, k
        assert k["lds_bytes"] == 0 and k["max_flat_workgroup_size"] == 64, k
