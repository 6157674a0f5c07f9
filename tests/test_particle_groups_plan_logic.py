"""CPU test of the host plans of the particle groups (csrc/avr_field_plans.h:
plan_particle_group_cells, plan_particle_groups); no GPU call.
tests/cxx/particle_groups_plan_test.cpp, built here with AddressSanitizer and UBSan, checks every
refusal message and which one wins, the 2^31, 2^27 and 1024 bounds from counts alone, the rule
h >= b (1 + 2^-10) at equality and one ulp below, 2 and 3 cells on a periodic axis, the shared-byte
rule to the byte, and the launch arguments against values written out by hand."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_particle_groups_plan_logic(tmp_path):
    program = str(tmp_path / "particle_groups_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "particle_groups_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
