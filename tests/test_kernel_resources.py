"""CPU-side gate on the register / scratch figures of the built gfx950 code objects (tools/kernel_resources.py reads the
NT_AMDGPU_METADATA notes out of libpphip.so; no GPU needed).  Round 1 shipped k_wavefront with 328 B of scratch per lane
(70 VGPR spills, 28 scratch stores per window cell inside the round loop); the figures below are what the restructured
kernels need and must not creep back up.  The planner's allocation headroom (pp_planner.hip: kMaxPrivateBytes) has to
cover the largest private segment of the kernels it launches."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# kernel -> (max scratch bytes per lane, max VGPR spills)
LIMITS = {
    "k_wavefront<false>": (176, 43),  # v10 (no up-front +inf fill; measured 174 -> 168 ms for 4096 goals with these figures)
    "k_hybrid_search_rows<false>": (384, 77),  # the batch form: unchanged by the pipeline form next to it
    "k_hybrid_search_rows<true>": (528, 113),  # the pipeline form (ring claims, completion records, idle handling); 310 of its 347 scratch loads sit in the
    # Reeds-Shepp block (0.9 % of the expansions), 26 in the per-expansion phases: tools/isa_spill_map.py, profiles/r04_search_spill_map.txt
    "k_hybrid_search<false>": (112, 0),
    "k_check_states": (0, 0),
    "k_check_states_fused": (0, 0),
    "k_check_arcs": (0, 0),
    "k_check_segments": (0, 0),
    "k_rollout": (0, 0),
    "k_rs_solve": (0, 0),
    "k_nonholo_build": (0, 0),
    "k_knn": (0, 0),
    "k_rrt": (0, 0),
    "k_grid_astar": (0, 0),
}


def test_scratch_and_spills_do_not_regress():
    from pathplanning_amd import build
    import kernel_resources
    lib = build.build(verbose=False)
    res = {k["kernel"]: k for k in kernel_resources.resources(lib)}
    for name, (scratch, spills) in LIMITS.items():
        assert name in res, (name, sorted(res))
        k = res[name]
        assert k["scratch_bytes_per_lane"] <= scratch, (name, k)
        assert k["vgpr_spill"] <= spills, (name, k)
    # the tile form of the wavefront (all instantiations): no scratch at all, and few enough registers for two waves beside a 256-register search wave on a SIMD
    # (512 registers per lane and SIMD, allocated in blocks of eight: 256 + 2 x 128; a third wave would need <= 80)
    tiles = [k for k in kernel_resources.resources(lib) if k["kernel"].startswith("k_wavefront_tiles")]
    assert len(tiles) >= 6  # tile widths 32 / 64 x {plain, counters, queue in global memory}
    for k in tiles:
        assert k["scratch_bytes_per_lane"] == 0 and k["vgpr_spill"] == 0 and k["vgpr"] <= 128, k
    # the wavefront kernel must keep two workgroups of eight waves per CU: <= 128 VGPRs, <= 80 KiB LDS
    assert res["k_wavefront<false>"]["vgpr"] <= 128 and res["k_wavefront<false>"]["lds_bytes"] <= 80 * 1024


def test_planner_headroom_covers_the_largest_private_segment():
    from pathplanning_amd import build
    import kernel_resources
    lib = build.build(verbose=False)
    res = {k["kernel"]: k for k in kernel_resources.resources(lib)}
    src = open(os.path.join(ROOT, "pathplanning_amd", "csrc", "pp_planner.hip")).read()
    reserve = int(re.search(r"constexpr size_t kMaxPrivateBytes = (\d+);", src).group(1))
    launched = [k for n, k in res.items() if n.startswith(("k_wavefront", "k_hybrid_search", "k_postprocess"))]
    assert launched and reserve >= max(k["scratch_bytes_per_lane"] for k in launched)


def test_search_kernel_scratch_stays_out_of_the_expansion_path(tmp_path):
    """What an expansion waits for is scratch traffic INSIDE its chain, not the kernel's spill count (with launch bounds of 3 / 4 waves
    per SIMD the pop, node and children phases get 43-78 scratch loads each and the same grid runs at 17.7 / 13.4 k plans/s instead of 27.2 k).  The pipeline form's
    listing (hipcc -S with line tables) is attributed to the phases between the kernel's own ROWS_STAMP markers (tools/isa_spill_map.py): the per-expansion phases
    together hold 23 scratch loads and 1 store today; the Reeds-Shepp block (0.9 % of the expansions) holds the other 300."""
    import subprocess
    import isa_spill_map
    from pathplanning_amd import build
    csrc = os.path.join(ROOT, "pathplanning_amd", "csrc")
    listing = str(tmp_path / "planner.s")
    flags = [f for f in build.FLAGS if f not in ("-fPIC", "-shared")]
    subprocess.check_call([build.hipcc()] + flags + ["-gline-tables-only", "-S", "--cuda-device-only", "-o", listing, os.path.join(csrc, "pp_planner.hip")],
                          stderr=subprocess.DEVNULL)
    phases = isa_spill_map.phases_from_stamps(os.path.join(csrc, "pp_planner_rows.hpp"))
    m = isa_spill_map.spill_map(listing, "k_hybrid_search_rowsILb1E", "pp_planner_rows.hpp", phases)
    hot = ("pop+refill", "node", "children", "insertion", "node-records")
    assert all(m[p][0] > 0 for p in hot if p != "node-records"), m  # (the attribution found the phases)
    loads, stores = sum(m[p][1] for p in hot), sum(m[p][2] for p in hot)
    assert loads <= 40 and stores <= 6, m
    assert m["reeds-shepp"][1] > loads  # the spills live where they cost nothing
