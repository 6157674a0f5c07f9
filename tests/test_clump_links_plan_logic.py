"""CPU test of the host plan of the clump links (csrc/avr_field_plans.h: plan_clump_links); no GPU
call.  tests/cxx/clump_links_plan_test.cpp, built here with AddressSanitizer and UBSan, checks every
refusal message and which one wins, the refined first cell and R_l of every box, the refined-extent
rule at its limit from descriptors alone, n_parents against the presence of a parent scene, and the
launch arguments and the order of visit_tables against values written out by hand."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_clump_links_plan_logic(tmp_path):
    program = str(tmp_path / "clump_links_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "clump_links_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
