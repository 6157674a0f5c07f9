"""CPU test of the host plan of the covering grids (csrc/avr_field_plans.h: plan_covering_grid); no
GPU call.  tests/cxx/covering_grid_plan_test.cpp, built here with AddressSanitizer and UBSan,
checks every refusal message and which one wins, the 2^31 and 2^30 rules from descriptors alone,
the weights w_m, the tiles' number and decode against cell_tile_of for ragged dims, and every
tile's candidate list against an enumeration of the tile's cells, their ancestors and their
descendants."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_covering_grid_plan_logic(tmp_path):
    program = str(tmp_path / "covering_grid_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "covering_grid_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
