"""CPU test of the host plan of ray transfer (csrc/avr_field_plans.h: plan_ray_transfer); no GPU
call.  tests/cxx/ray_transfer_plan_test.cpp, built here with AddressSanitizer and UBSan, checks
every refusal message and which one wins, the three extra scenes' rules, 1024 and 1025 channels,
the limit on channels x rays, the chunk arithmetic, the reciprocals' bits, the shared-byte rule to
the byte, and that a plan holds plan_ray_sums' walk tables entry for entry."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_ray_transfer_plan_logic(tmp_path):
    program = str(tmp_path / "ray_transfer_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "ray_transfer_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
