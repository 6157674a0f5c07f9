"""CPU test of the host plans of the power spectra (csrc/avr_field_plans.h: plan_fft3d,
plan_spectrum_bins); no GPU call.  tests/cxx/fft_plan_test.cpp, built here with AddressSanitizer
and UBSan, checks every refusal message and which one wins, the 1024, 2^31 and 2048 limits, the
overlap rules to the byte, the passes' strides and column groups with a last, partial group, the
launch shapes of the sixteen grids of test_fft_lengths.py written out by hand (with the two that
stage exactly 64 KiB), and the twiddle table for n = 2, 8 and 1024 against cos and sin."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_fft_plan_logic(tmp_path):
    program = str(tmp_path / "fft_plan_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "fft_plan_test.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
