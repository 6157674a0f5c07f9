"""CPU test of the host plan of the grid fields (csrc/avr_field_plans.h: plan_grid_field); no GPU
call.  tests/cxx/grid_field_plan_test.cpp, built here with AddressSanitizer and UBSan, checks
every refusal message and which one wins, the 2^30 and 2^31 rules from descriptors alone, the
shared-byte rule to the byte, and the launch arguments and staged tables against values written
out by hand."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_grid_field_plan_logic(tmp_path):
    program = str(tmp_path / "grid_field_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "grid_field_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
