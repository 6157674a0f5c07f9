"""CPU test of the host plans of the isolated potential (csrc/avr_field_plans.h:
plan_isolated_green, plan_spectrum_multiply); no GPU call.  tests/cxx/isolated_plan_test.cpp, built
here with AddressSanitizer and UBSan, checks every refusal message and which one wins, the limits
of the cell size at DBL_MIN and at overflow, the overlap rule of the two spectra to the byte, the
cell count at 2^30 and at 2^31, and the launch shape for padded grids of (1, 1, 1), (4, 1, 1) and
(1024, 1024, 1024)."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_isolated_plan_logic(tmp_path):
    program = str(tmp_path / "isolated_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "isolated_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
