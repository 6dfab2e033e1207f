"""CPU-side gate on the SIZE and LAYOUT of the rows kernels' code (no GPU needed; built and listed the way tests/test_kernel_resources.py does).
Eight search waves per pair of compute units run the expansion loop out of one 64 KB instruction cache, next to tile waves with 13.4 KB of
their own, so what a row enters rarely lives in called functions (pathplanning_amd/csrc/pp_rows_rs.hpp) and the loop's text must not creep
back up ("code size and layout"; profiles/search_code_layout.txt).

Before the change k_hybrid_search_rows<true> was 171 668 B with 9 554 instructions in its per-expansion phases (9.8 k with the code the
listing attributes to no line of the body); every gate below is the finished build's figure plus 5 %, and far below those.  Per-expansion
code of the pipeline form: 6 801 instructions x 5.9 B = 40 KB, + 13.4 KB of the tile kernel = 53.5 KB of the 64 KB cache."""
import os
import re
import struct
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOT = ("pop+refill", "node", "children", "insertion", "node-records")
BODY = "pp_planner_rows.hpp"

# kernel (as its mangled name spells it) -> (measured symbol size in bytes, gate), (measured per-expansion instructions incl. called functions, gate)
KERNELS = {
    "k_hybrid_search_rowsILb0E": ((56_724, 59_560), (6_685, 7_019)),            # batch form
    "k_hybrid_search_rowsILb1E": ((54_716, 57_452), (6_801, 7_141)),            # pipeline form: the bench's steady state
    "k_hybrid_search_rows_footprintILb1E": ((68_720, 72_156), (8_547, 8_974)),  # pipeline form with a vehicle footprint
}
# the Reeds-Shepp attempt, by validator form: rows_rs_attempt<false> (point) 38 016 B, <true> (footprint) 42 964 B
RS_ATTEMPTS = ("rows_rs_attemptILb0E", "rows_rs_attemptILb1E")
PARENT_BYTES, PARENT_HOT_INSTS = 171_668, 9_800


def symbol_sizes(lib):
    """{symbol: size} of the functions in the gfx950 code objects of the library"""
    import kernel_resources
    out = {}
    for elf in kernel_resources.code_objects(lib):
        (symoff, symsize, _), = kernel_resources._section(elf, ".symtab")
        (stroff, _, _), = kernel_resources._section(elf, ".strtab")
        for p in range(symoff, symoff + symsize, 24):
            name, info, _, _, _, size = struct.unpack_from("<IBBHQQ", elf, p)
            if (info & 0xF) == 2 and size:  # STT_FUNC
                out[elf[stroff + name:elf.index(b"\0", stroff + name)].decode()] = size
    return out


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from pathplanning_amd import build
    csrc = os.path.join(ROOT, "pathplanning_amd", "csrc")
    path = str(tmp_path_factory.mktemp("layout") / "planner.s")
    flags = [f for f in build.FLAGS if f not in ("-fPIC", "-shared")]
    subprocess.check_call([build.hipcc()] + flags + ["-gline-tables-only", "-S", "--cuda-device-only", "-o", path, os.path.join(csrc, "pp_planner.hip")],
                          stderr=subprocess.DEVNULL)
    return path, open(path).read().split("\n")


INST = re.compile(r"(v_|s_|ds_|global_|scratch_|buffer_|flat_)")
FRAME = re.compile(r"([\w./+-]+):(\d+):\d+")


def function_body(lines, label):
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and label in l and ": " in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end]


def instructions(lines, label):
    return sum(1 for l in function_body(lines, label) if INST.match(l.strip()))


def functions_called_between(lines, kernel, lo, hi):
    """the functions whose address the kernel takes (to call them) in code attributed to lines lo..hi of its body, attributed as
    tools/isa_spill_map.py attributes instructions"""
    cur, out = None, set()
    for l in function_body(lines, kernel):
        s = l.strip()
        if s.startswith(".loc"):
            c = s.split(";", 1)[1] if ";" in s else ""
            inb = [int(n) for f, n in FRAME.findall(c) if f.split("/")[-1] == BODY and int(n) > 0]
            cur = inb[-1] if inb else cur
            continue
        m = re.search(r"(_Z\w+)@rel32@lo", s)
        if m and cur is not None and lo <= cur <= hi:
            out.add(m.group(1))
    return out


def test_the_reeds_shepp_attempt_is_a_function_of_its_own_and_the_kernels_stay_small():
    from pathplanning_amd import build
    sizes = symbol_sizes(build.build(verbose=False))
    for rs in RS_ATTEMPTS:  # both validator forms; the batch and the pipeline form of a validator call the same function
        hit = [n for n in sizes if rs in n]
        assert len(hit) == 1 and sizes[hit[0]] > 0, (rs, hit)
        assert "k_hybrid_search_rows" not in hit[0]  # (tools/isa_spill_map.py finds a kernel by the first label that contains its name)
    for kernel, ((_, gate), _) in KERNELS.items():
        hit = [n for n in sizes if kernel in n and not n.endswith(".kd")]
        assert len(hit) == 1, (kernel, hit)
        print(kernel, sizes[hit[0]], "bytes; gate", gate)
        assert gate < PARENT_BYTES
        assert sizes[hit[0]] <= gate, (kernel, sizes[hit[0]], gate)


@pytest.mark.parametrize("kernel", sorted(KERNELS))
def test_the_per_expansion_code_stays_small(listing, kernel):
    import isa_spill_map
    phases = isa_spill_map.phases_from_stamps(os.path.join(ROOT, "pathplanning_amd", "csrc", BODY))
    path, lines = listing
    m = isa_spill_map.spill_map(path, kernel, BODY, phases)
    assert all(m[p][0] > 0 for p in HOT), m  # (the attribution found the phases)
    hot = sum(m[p][0] for p in HOT)
    lo, hi = min(p[1] for p in phases if p[0] in HOT), max(p[2] for p in phases if p[0] in HOT)
    called = {f: instructions(lines, f) for f in functions_called_between(lines, kernel, lo, hi)}
    assert all("rows_rs_attempt" not in f and "rows_claim_init" not in f for f in called), called  # the cold pieces are not entered from the hot phases
    total = hot + sum(called.values())
    (_, (_, gate)) = KERNELS[kernel]
    print(kernel, "per-expansion instructions", hot, "+ called", called, "=", total, "; gate", gate)
    assert gate < PARENT_HOT_INSTS
    assert total <= gate, (kernel, total, gate, m)
