"""CPU test of the host plans of the clump members (csrc/avr_field_plans.h: plan_clump_members and
plan_clump_member_data); no GPU call.  tests/cxx/clump_members_plan_test.cpp, built here with
AddressSanitizer and UBSan, checks every refusal message and which one wins, the cell ordinals of
boxes with and without cells, the 2^31-cell rule at its limit from descriptors alone, and the
launch arguments, the box tables and the order of visit_tables against values written out by
hand."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_clump_members_plan_logic(tmp_path):
    program = str(tmp_path / "clump_members_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "clump_members_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
