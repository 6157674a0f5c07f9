"""CPU test of the same-or-coarser cell lookup (csrc/avr_level_cells.h: find_same_or_coarser), the
one definition the gradient's halo and the isosurfaces' shell call in their kernels (the clumps'
unite_ghost writes the same loop out); no GPU call. tests/cxx/level_cells_test.cpp, built here with
AddressSanitizer and UBSan, runs it over every cell of every box's one-cell shell of a three-level
scene (negative indices, a hole that a coarser level covers, a ghost no box holds, a box without
cells, boxes that touch) through the candidate lists of plan_isosurface, plan_clumps and
plan_gradient, and holds every result against a scan of all boxes."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_level_cells_logic(tmp_path):
    program = str(tmp_path / "level_cells_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "level_cells_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
