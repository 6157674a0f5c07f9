"""CPU test of the host plan of the structure functions (csrc/avr_field_plans.h:
plan_structure_functions); no GPU call.  tests/cxx/structure_plan_test.cpp, built here with
AddressSanitizer and UBSan, checks every refusal message and which one wins, the limits of 4096
lags and order 8, a lag of N_d - 1 admitted and one of N_d refused in both boundary modes, dims of
(2^31 - 1, 1, 1) admitted and 2^31 cells refused from the descriptors alone, the shared-byte rule
to the byte for each output against each component and among the outputs, and the staged table
and the launch shape written out by hand."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_structure_plan_logic(tmp_path):
    program = str(tmp_path / "structure_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "structure_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
