"""CPU test of the host plan of the rays (csrc/avr_field_plans.h: plan_rays); no GPU call.
tests/cxx/ray_plan_test.cpp, built here with AddressSanitizer and UBSan, checks every refusal
message and which one wins, the size rules from descriptors alone, and that the locator the
factored-out construction builds for plan_rays is plan_streamlines' for the same boxes, with
[Blo, Bhi] the boxes' hull at level 0."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_ray_plan_logic(tmp_path):
    program = str(tmp_path / "ray_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "ray_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
