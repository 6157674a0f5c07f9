"""CPU test of the host plan of the velocity cubes (csrc/avr_field_plans.h: plan_velocity_cube); no
GPU call.  tests/cxx/velocity_cube_plan_test.cpp, built here with AddressSanitizer and UBSan,
checks every refusal message and which one wins, 1024 channels admitted and 1025 refused, the limit
on channels x width x height, the batch arithmetic at entries x channels equal to the scratch bound
and one above it, a forced bound that gives batches of one channel, the shared-byte rule to the
byte and the staged tables and launch arguments written out by hand."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_velocity_cube_plan_logic(tmp_path):
    program = str(tmp_path / "velocity_cube_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "velocity_cube_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
