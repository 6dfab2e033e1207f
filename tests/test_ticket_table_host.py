"""CPU: the streaming pipeline's slot and ticket bookkeeping (pathplanning_amd/csrc/pp_ticket_table.hpp) alone, through tests/cpp/test_ticket_table.cpp -- a
stand-alone program built with g++ under the address and undefined-behaviour sanitizers: hand-out order, no room, hold / release / reuse with the generation
advanced, refused completions, resolve()'s refusals by name (and that they change nothing), and one slot through kGenMask + 2 fills."""
import subprocess


def test_the_ticket_table_program_passes_under_the_sanitizers():
    from pathplanning_amd import build
    exe = build.build_ticket_table_test(verbose=False)
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert "ticket table ok" in run.stdout
