"""CPU test of the host plans of the clumps (csrc/avr_field_plans.h: plan_clumps and
plan_clump_table); no GPU call.  tests/cxx/clump_plan_test.cpp, built here with AddressSanitizer
and UBSan, checks every refusal message and which one wins, cell_begin, the 2^31-cell rule from
descriptors alone, the table's n_clumps * n_levels limit and the candidate lists of all six faces
against an enumeration of every ghost cell and its ancestors."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_clump_plan_logic(tmp_path):
    program = str(tmp_path / "clump_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "clump_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
