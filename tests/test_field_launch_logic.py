"""CPU test of what the field products' plans hand to their entry points (csrc/avr_field_plans.h ->
csrc/avr_field_products.cpp); no GPU call.  tests/cxx/field_launch_test.cpp, built with
AddressSanitizer and UBSan, checks for all twelve products the launch arguments a plan fills (and
that it leaves every device address null), the tables it names for staging with their order, element
sizes and counts -- an empty one is sized as one element by the stager's sizing pass -- and the
scratch layouts against the formulae the entry points used to spell out."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_field_launch_logic():
    subprocess.run(["make", "-C", CXX, "field_launch_test"], check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(CXX, "field_launch_test")], capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
