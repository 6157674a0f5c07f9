"""CPU test of the four-instruction bricklet offset (csrc/avr_brick_address.h: pow2_brick_shifts,
pow2_brick_keys, pow2_brick_offset), the one definition the march's interior loops call for boxes
whose bricklet counts are powers of two (IndexMode kPow2Bricks); no GPU call.
tests/cxx/pow2_brick_address_test.cpp, built here with AddressSanitizer and UBSan together with the
host prologue (csrc/avr_host.cpp), holds it against bricklet_offset's formula for every cell of 8^3,
16^3, 64^3, 20 x 16 x 13 (partial bricklets) and 256 x 16 x 16 (nx at its bound) and for a sample of
128^3's, each with the five fraction bits under the z index at 0, 13 and 31; checks that 257 x 16 x
16, 16 x 24 x 16, 16 x 17 x 16, 16 x 16 x 4 and 8 x 32 x 8 do not qualify; and that plan_frame gives
qualifying power-of-two boxes the new mode, their neighbours kPow2Multiply and a box of another
spacing kReciprocal."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")
CSRC = os.path.join(os.path.dirname(CXX), os.pardir, "amrvolumerenderer_amd", "csrc")


def test_pow2_brick_address(tmp_path):
    program = str(tmp_path / "pow2_brick_address_test")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra",
                    "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", program, os.path.join(CXX, "pow2_brick_address_test.cpp"),
                    os.path.join(CSRC, "avr_host.cpp")], check=True)
    out = subprocess.run([program], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
