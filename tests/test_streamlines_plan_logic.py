"""CPU test of the host plan of the streamlines (csrc/avr_field_plans.h: plan_streamlines); no GPU
call.  tests/cxx/streamlines_plan_test.cpp, built here with AddressSanitizer and UBSan, checks every
refusal message and which one wins, the size rules from descriptors alone, and the locator against
brute force: for every cell of every box and of every box's one-cell ghost shell, the block's list
holds every box a scan of all boxes finds, in the required order, and a walk of it ends where the
scan ends."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_streamlines_plan_logic(tmp_path):
    program = str(tmp_path / "streamlines_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "streamlines_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
