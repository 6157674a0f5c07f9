"""CPU test of the host plan of the isosurfaces (csrc/avr_field_plans.h: plan_isosurface); no GPU
call.  tests/cxx/isosurface_plan_test.cpp, built here with AddressSanitizer and UBSan, checks every
refusal message and which one wins, base_begin and shell_begin, the numbering of the shell cells,
the 2^31 rule from descriptors alone, the region candidates against an enumeration of every shell
cell and its ancestors, and that the face candidates of the clumps and the gradient are what an
enumeration of the faces' ghost cells gives."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_isosurface_plan_logic(tmp_path):
    program = str(tmp_path / "isosurface_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "isosurface_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
