"""CPU-side gate on the three kernels of a delay call with tracked movers (pathplanning_amd/csrc/pp_tracks.hpp): they are in the built gfx950 code
object, take no scratch and spill nothing (tools/kernel_resources.py reads the figures out of libpphip.so; no GPU needed).  k_delay_level, whose
partner scan k_delay_level_tracks restates, has 58 VGPRs and no scratch; these do no more per lane."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

KERNELS = ("k_track_samples", "k_delay_level_tracks", "k_track_pairs")


def test_the_three_kernels_are_built_without_scratch_or_spills():
    from pathplanning_amd import build
    import kernel_resources
    res = {k["kernel"]: k for k in kernel_resources.resources(build.build(verbose=False))}
    for name in KERNELS:
        assert name in res, (name, sorted(res))
        k = res[name]
        print(name, k)
        assert k["scratch_bytes_per_lane"] == 0 and k["vgpr_spill"] == 0, k
        assert k["lds_bytes"] == 0, k
