"""CPU test of the host plans of the field products (csrc/avr_field_plans.h: slice images, the
joint histogram, on-axis projections, derived fields, gradient fields); no GPU call in any.
tests/cxx/field_plans_test.cpp, built with AddressSanitizer and UBSan, checks the derive program's
verifier, the shared-byte rule, the gradient's neighbour lists against an enumeration of the ghost
cells, the projection's plane tables, the histogram's edge rules and every refusal message."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_field_plans_logic():
    subprocess.run(["make", "-C", CXX, "field_plans_test"], check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(CXX, "field_plans_test")], capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
