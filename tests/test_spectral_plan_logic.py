"""CPU test of the host plans of the inverse transform and the per-mode operators
(csrc/avr_field_plans.h: plan_ifft3d, plan_spectrum_helmholtz, plan_spectrum_inverse_laplacian); no
GPU call.  tests/cxx/spectral_plan_test.cpp, built here with AddressSanitizer and UBSan, checks
every refusal message and which one wins, the overlap rules to the byte among three and among six
arrays, the limits of h at DBL_MIN and at overflow, the inverse table against the forward one for
n = 2, 8 and 1024, and the x pass's cut for nx = 1, 2 and 1024."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_spectral_plan_logic(tmp_path):
    program = str(tmp_path / "spectral_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "spectral_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
