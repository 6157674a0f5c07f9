"""CPU test of the host plan of the per-ray sums (csrc/avr_field_plans.h: plan_ray_sums); no GPU
call.  tests/cxx/ray_sums_plan_test.cpp, built here with AddressSanitizer and UBSan, checks every
refusal message and which one wins, the weight scene's rules, the shared-byte rule over the new
outputs and the weight's cells, and that a plan without a weight holds plan_rays' tables entry for
entry."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_ray_sums_plan_logic(tmp_path):
    program = str(tmp_path / "ray_sums_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "ray_sums_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
