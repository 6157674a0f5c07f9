"""CPU test of the host plan of the pairwise self-energy (csrc/avr_field_plans.h: plan_clump_pairs);
no GPU call.  tests/cxx/clump_pairs_plan_test.cpp, built here with AddressSanitizer and UBSan,
checks every refusal message and which one wins, the items of segments of 0, 1, 2, 255, 256, 257,
513, 4099 and past the cap of 64 j tiles, that every tile pair is covered exactly once, that the
partial ranges are contiguous per segment, that depth <= N + 64 for every segment -- what keeps the
GPU test's tolerance from being inflated by the code under test -- and the limits at 2^22 and 2^31
from offsets alone."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_clump_pairs_plan_logic(tmp_path):
    program = str(tmp_path / "clump_pairs_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "clump_pairs_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
