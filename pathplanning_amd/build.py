"""Builds libpphip.so (HIP, gfx950) in-tree: pathplanning_amd/lib/libpphip.so."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIB_DIR, "libpphip.so")
SOURCES = ["pp_capi.hip", "pp_kernels_basic.hip", "pp_paths.hip", "pp_footprint.hip", "pp_gvd.hip", "pp_wavefront.hip", "pp_wavefront_tiles.hip", "pp_planner.hip", "pp_rrt.hip", "pp_grid_astar.hip"]
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".hpp")) + [os.path.join("..", "..", "include", "pp_hip.h")]
# -ffp-contract=off: no FMA contraction -- discrete outputs must match the CPU reference bit for bit.
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]


def hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def stale():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS]
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    if not force and not stale():
        return LIB
    os.makedirs(LIB_DIR, exist_ok=True)
    extra = os.environ.get("PP_EXTRA_HIPCC_FLAGS", "").split()  # tuning experiments, e.g. -DPP_WF_WAVES_PER_SIMD=2
    cmd = [hipcc()] + FLAGS + extra + ["-o", LIB] + [os.path.join(CSRC, s) for s in SOURCES]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd, cwd=CSRC)
    return LIB


def build_pyplanning(force=False, verbose=True):
    """pybind11 module `pyplanning` (reference's Python surface for the hot path), linked against libpphip.so."""
    import sysconfig
    import pybind11
    build()
    host = os.path.join(HERE, "host")
    ext = sysconfig.get_config_var("EXT_SUFFIX") or ".so"
    out = os.path.join(LIB_DIR, "pyplanning" + ext)
    srcs = [os.path.join(host, f) for f in sorted(os.listdir(host)) if f.endswith((".cpp", ".hpp"))] + [os.path.join(HERE, "..", "include", "pp_hip.h")]
    if not force and os.path.exists(out) and all(os.path.getmtime(x) <= os.path.getmtime(out) for x in srcs):
        return out
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-fvisibility=hidden", "-I" + pybind11.get_include(), "-I" + sysconfig.get_paths()["include"],
           os.path.join(host, "pyplanning.cpp"), "-o", out, "-L" + LIB_DIR, "-lpphip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_plugin_test(verbose=True):
    """tests/cpp/test_plugin.cpp against the C++ plugin header (run on the GPU box)."""
    build()
    out = os.path.join(LIB_DIR, "test_plugin")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_plugin.cpp")
    cmd = ["g++", "-O2", "-std=c++17", src, "-o", out, "-L" + LIB_DIR, "-lpphip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_pipeline_footprint_test(verbose=True):
    """tests/cpp/test_pipeline_footprint.cpp: the validator's footprint through HybridAStarPipeline (run on the GPU box)."""
    build()
    out = os.path.join(LIB_DIR, "test_pipeline_footprint")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_pipeline_footprint.cpp")
    cmd = ["g++", "-O2", "-std=c++17", src, "-o", out, "-L" + LIB_DIR, "-lpphip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_pipeline_postprocess_test(verbose=True):
    """tests/cpp/test_pipeline_postprocess.cpp: GetPath(ticket) of HybridAStarPipeline against HybridAStar::SearchPath + GetPath (run on the GPU box)."""
    build()
    out = os.path.join(LIB_DIR, "test_pipeline_postprocess")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_pipeline_postprocess.cpp")
    cmd = ["g++", "-O2", "-std=c++17", src, "-o", out, "-L" + LIB_DIR, "-lpphip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_pipeline_revalidate_test(verbose=True):
    """tests/cpp/test_pipeline_revalidate.cpp: Revalidate(tickets) of HybridAStarPipeline against the plan's path objects marched one by one (run on the GPU box)."""
    build()
    out = os.path.join(LIB_DIR, "test_pipeline_revalidate")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_pipeline_revalidate.cpp")
    cmd = ["g++", "-O2", "-std=c++17", src, "-o", out, "-L" + LIB_DIR, "-lpphip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_pipeline_stamp_test(verbose=True):
    """tests/cpp/test_pipeline_stamp.cpp: Stamp(tickets) of HybridAStarPipeline against the plan's path objects sampled and rasterised one by one (run on the GPU box)."""
    build()
    out = os.path.join(LIB_DIR, "test_pipeline_stamp")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_pipeline_stamp.cpp")
    cmd = ["g++", "-O2", "-std=c++17", src, "-o", out, "-L" + LIB_DIR, "-lpphip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_stamp_rule_test(verbose=True):
    """tests/cpp/test_stamp_rule.cpp: the stamp's sample schedule and cell rule (csrc/pp_stamp_rule.hpp) alone, on the CPU, under the address and
    undefined-behaviour sanitizers; without contraction, as the library is built."""
    os.makedirs(LIB_DIR, exist_ok=True)
    out = os.path.join(LIB_DIR, "test_stamp_rule")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_stamp_rule.cpp")
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(src), os.path.getmtime(os.path.join(CSRC, "pp_stamp_rule.hpp"))):
        return out
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_pipeline_locate_test(verbose=True):
    """tests/cpp/test_pipeline_locate.cpp: Locate(tickets, poses) of HybridAStarPipeline against the plan's path objects searched point by point (run on the GPU box)."""
    build()
    out = os.path.join(LIB_DIR, "test_pipeline_locate")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_pipeline_locate.cpp")
    cmd = ["g++", "-O2", "-std=c++17", src, "-o", out, "-L" + LIB_DIR, "-lpphip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_locate_rule_test(verbose=True):
    """tests/cpp/test_locate_rule.cpp: the wrap, the cost, the order, the lattice and the arc length -> (edge, ratio) mapping of a locate call
    (csrc/pp_locate_rule.hpp) alone, on the CPU, under the address and undefined-behaviour sanitizers; without contraction, as the library is built."""
    os.makedirs(LIB_DIR, exist_ok=True)
    out = os.path.join(LIB_DIR, "test_locate_rule")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_locate_rule.cpp")
    headers = [os.path.join(CSRC, "pp_locate_rule.hpp"), os.path.join(CSRC, "pp_stamp_rule.hpp")]
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(f) for f in [src] + headers):
        return out
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_pipeline_speed_profile_test(verbose=True):
    """tests/cpp/test_pipeline_speed_profile.cpp: SpeedProfile(tickets) of HybridAStarPipeline against a sequential sweep over the plan's path objects (run on the GPU box)."""
    build()
    out = os.path.join(LIB_DIR, "test_pipeline_speed_profile")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_pipeline_speed_profile.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", out, "-L" + LIB_DIR, "-lpphip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_speed_rule_test(verbose=True):
    """tests/cpp/test_speed_rule.cpp: the cap, the envelopes, the step time and the cusp predicate of a speed profile (csrc/pp_speed_rule.hpp) alone, on
    the CPU, under the address and undefined-behaviour sanitizers; without contraction, as the library is built."""
    os.makedirs(LIB_DIR, exist_ok=True)
    out = os.path.join(LIB_DIR, "test_speed_rule")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_speed_rule.cpp")
    headers = [os.path.join(CSRC, "pp_speed_rule.hpp"), os.path.join(CSRC, "pp_stamp_rule.hpp")]
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(f) for f in [src] + headers):
        return out
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_pipeline_conflicts_test(verbose=True):
    """tests/cpp/test_pipeline_conflicts.cpp: Conflicts(tickets, starts) of HybridAStarPipeline against a plain sequential loop over the profile rows and the plan's
    path objects (run on the GPU box)."""
    build()
    out = os.path.join(LIB_DIR, "test_pipeline_conflicts")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_pipeline_conflicts.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", out, "-L" + LIB_DIR, "-lpphip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_conflict_rule_test(verbose=True):
    """tests/cpp/test_conflict_rule.cpp: the lattice, the row search, the position within a step, the separation and the two orders of a conflict call
    (csrc/pp_conflict_rule.hpp) alone, on the CPU, under the address and undefined-behaviour sanitizers; without contraction, as the library is built."""
    os.makedirs(LIB_DIR, exist_ok=True)
    out = os.path.join(LIB_DIR, "test_conflict_rule")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_conflict_rule.cpp")
    headers = [os.path.join(CSRC, "pp_conflict_rule.hpp"), os.path.join(CSRC, "pp_speed_rule.hpp"), os.path.join(CSRC, "pp_stamp_rule.hpp")]
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(f) for f in [src] + headers):
        return out
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_pipeline_deconflict_test(verbose=True):
    """tests/cpp/test_pipeline_deconflict.cpp: Deconflict(tickets, starts) of HybridAStarPipeline against a plain sequential loop over the poses Conflicts returns
    (run on the GPU box)."""
    build()
    out = os.path.join(LIB_DIR, "test_pipeline_deconflict")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_pipeline_deconflict.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", out, "-L" + LIB_DIR, "-lpphip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_delay_rule_test(verbose=True):
    """tests/cpp/test_delay_rule.cpp: the column of a delayed vehicle, the key of a conflict, the partner lists and the levels of a delay call
    (csrc/pp_delay_rule.hpp) alone, on the CPU, under the address and undefined-behaviour sanitizers."""
    os.makedirs(LIB_DIR, exist_ok=True)
    out = os.path.join(LIB_DIR, "test_delay_rule")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_delay_rule.cpp")
    headers = [os.path.join(CSRC, "pp_delay_rule.hpp"), os.path.join(CSRC, "pp_conflict_rule.hpp"), os.path.join(CSRC, "pp_speed_rule.hpp"), os.path.join(CSRC, "pp_stamp_rule.hpp")]
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(f) for f in [src] + headers):
        return out
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_pipeline_deconflict_tracks_test(verbose=True):
    """tests/cpp/test_pipeline_deconflict_tracks.cpp: DeconflictTracks(tickets, starts, tracks) of HybridAStarPipeline against a plain sequential loop over the poses
    Conflicts returns and the tracks' waypoints (run on the GPU box)."""
    build()
    out = os.path.join(LIB_DIR, "test_pipeline_deconflict_tracks")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_pipeline_deconflict_tracks.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", out, "-L" + LIB_DIR, "-lpphip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_track_rule_test(verbose=True):
    """tests/cpp/test_track_rule.cpp: the waypoint search, the position of a track, the partner index of a track and the validation of a track set
    (csrc/pp_track_rule.hpp) alone, on the CPU, under the address and undefined-behaviour sanitizers; without contraction, as the library is built."""
    os.makedirs(LIB_DIR, exist_ok=True)
    out = os.path.join(LIB_DIR, "test_track_rule")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_track_rule.cpp")
    headers = [os.path.join(CSRC, f) for f in ("pp_track_rule.hpp", "pp_delay_rule.hpp", "pp_conflict_rule.hpp", "pp_speed_rule.hpp", "pp_stamp_rule.hpp")]
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(f) for f in [src] + headers):
        return out
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_pipeline_candidate_pairs_test(verbose=True):
    """tests/cpp/test_pipeline_candidate_pairs.cpp: CandidatePairs(tickets, starts) of HybridAStarPipeline against a plain sequential loop over the poses
    Conflicts returns (run on the GPU box)."""
    build()
    out = os.path.join(LIB_DIR, "test_pipeline_candidate_pairs")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_pipeline_candidate_pairs.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", out, "-L" + LIB_DIR, "-lpphip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_pair_rule_test(verbose=True):
    """tests/cpp/test_pair_rule.cpp: the box count, a box's column range, the reach, the accumulation and merge of a box and the two-axis test
    (csrc/pp_pair_rule.hpp) alone, on the CPU, under the address and undefined-behaviour sanitizers; without contraction, as the library is built."""
    os.makedirs(LIB_DIR, exist_ok=True)
    out = os.path.join(LIB_DIR, "test_pair_rule")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_pair_rule.cpp")
    headers = [os.path.join(CSRC, "pp_pair_rule.hpp")]
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(f) for f in [src] + headers):
        return out
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_pipeline_timetable_test(verbose=True):
    """tests/cpp/test_pipeline_timetable.cpp: Timetable(tickets, values) of HybridAStarPipeline against a plain sequential loop over the rows SpeedProfile
    downloads (run on the GPU box)."""
    build()
    out = os.path.join(LIB_DIR, "test_pipeline_timetable")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_pipeline_timetable.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", out, "-L" + LIB_DIR, "-lpphip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_timetable_rule_test(verbose=True):
    """tests/cpp/test_timetable_rule.cpp: the row search by arc length, the inverse step, speed and acceleration by time, the stops and the next-stop
    search (csrc/pp_timetable_rule.hpp) alone, on the CPU, under the address and undefined-behaviour sanitizers; without contraction, as the library is
    built."""
    os.makedirs(LIB_DIR, exist_ok=True)
    out = os.path.join(LIB_DIR, "test_timetable_rule")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_timetable_rule.cpp")
    headers = [os.path.join(CSRC, h) for h in ("pp_timetable_rule.hpp", "pp_conflict_rule.hpp", "pp_speed_rule.hpp", "pp_stamp_rule.hpp")]
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(f) for f in [src] + headers):
        return out
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_pipeline_deconflict_waits_test(verbose=True):
    """tests/cpp/test_pipeline_deconflict_waits.cpp: DeconflictWaits(tickets, starts) of HybridAStarPipeline against a plain sequential loop over the poses Conflicts
    returns and the places the call returns (run on the GPU box)."""
    build()
    out = os.path.join(LIB_DIR, "test_pipeline_deconflict_waits")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_pipeline_deconflict_waits.cpp")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", src, "-o", out, "-L" + LIB_DIR, "-lpphip", "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_wait_rule_test(verbose=True):
    """tests/cpp/test_wait_rule.cpp: the arrive column, the position under a wait, the place filter, the candidate order and the shortcut's predicate
    (csrc/pp_wait_rule.hpp) alone, on the CPU, under the address and undefined-behaviour sanitizers; without contraction, as the library is built."""
    os.makedirs(LIB_DIR, exist_ok=True)
    out = os.path.join(LIB_DIR, "test_wait_rule")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_wait_rule.cpp")
    headers = [os.path.join(CSRC, "pp_wait_rule.hpp")]
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(f) for f in [src] + headers):
        return out
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_retime_rule_test(verbose=True):
    """tests/cpp/test_retime_rule.cpp: the dwell of a row, the validity of a hold, the prefix, the hold a row belongs to and the rewritten time
    (csrc/pp_retime_rule.hpp) alone, on the CPU, under the address and undefined-behaviour sanitizers; without contraction, as the library is built."""
    os.makedirs(LIB_DIR, exist_ok=True)
    out = os.path.join(LIB_DIR, "test_retime_rule")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_retime_rule.cpp")
    headers = [os.path.join(CSRC, h) for h in ("pp_retime_rule.hpp", "pp_timetable_rule.hpp", "pp_conflict_rule.hpp", "pp_speed_rule.hpp", "pp_stamp_rule.hpp")]
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(f) for f in [src] + headers):
        return out
    cmd = ["g++", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_ticket_table_test(verbose=True):
    """tests/cpp/test_ticket_table.cpp: the pipeline's slot and ticket bookkeeping (csrc/pp_ticket_table.hpp) alone, on the CPU, under the address and
    undefined-behaviour sanitizers."""
    os.makedirs(LIB_DIR, exist_ok=True)
    out = os.path.join(LIB_DIR, "test_ticket_table")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_ticket_table.cpp")
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(src), os.path.getmtime(os.path.join(CSRC, "pp_ticket_table.hpp"))):
        return out
    cmd = ["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src, "-o", out]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


def build_row_test(verbose=True):
    """tests/cpp/test_row_primitives.hip: GPU self-test of the DPP row primitives (run on the GPU box)."""
    out = os.path.join(LIB_DIR, "test_row_primitives")
    src = os.path.join(HERE, "..", "tests", "cpp", "test_row_primitives.hip")
    if os.path.exists(out) and os.path.getmtime(out) > max(os.path.getmtime(src), os.path.getmtime(os.path.join(CSRC, "pp_row_primitives.hpp"))):
        return out
    cmd = [hipcc(), "--offload-arch=gfx950", "-O2", "-I", CSRC, "-I", os.path.join(HERE, "..", "include"), src, "-o", out]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.check_call(cmd)
    return out


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
    print(build_pyplanning())
    print(build_plugin_test())
    print(build_pipeline_footprint_test())
    print(build_pipeline_postprocess_test())
    print(build_pipeline_revalidate_test())
    print(build_pipeline_stamp_test())
    print(build_stamp_rule_test())
    print(build_pipeline_locate_test())
    print(build_locate_rule_test())
    print(build_pipeline_speed_profile_test())
    print(build_speed_rule_test())
    print(build_pipeline_conflicts_test())
    print(build_conflict_rule_test())
    print(build_pipeline_deconflict_test())
    print(build_delay_rule_test())
    print(build_pipeline_deconflict_tracks_test())
    print(build_track_rule_test())
    print(build_pipeline_candidate_pairs_test())
    print(build_pair_rule_test())
    print(build_pipeline_timetable_test())
    print(build_timetable_rule_test())
    print(build_pipeline_deconflict_waits_test())
    print(build_wait_rule_test())
    print(build_retime_rule_test())
    print(build_ticket_table_test())
    print(build_row_test())
