"""CPU test of the host plans of the particle fields (csrc/avr_field_plans.h: plan_particle_cells,
plan_particle_deposit); no GPU call.  tests/cxx/particles_plan_test.cpp, built here with
AddressSanitizer and UBSan, checks every refusal message and which one wins, the 2^28 and 2^31
bounds from counts alone, the shared-byte rule to the byte, and the staged tables (box table, cell
prefix, locator, tile prefix, volumes) against values written out by hand."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_particles_plan_logic(tmp_path):
    program = str(tmp_path / "particles_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "particles_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
