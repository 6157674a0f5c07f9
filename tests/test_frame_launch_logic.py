"""CPU test of what a frame's launch plan hands to render() (csrc/avr_frame_launch.h ->
csrc/avr_capi.cpp); no GPU call.  tests/cxx/frame_launch_test.cpp, built with AddressSanitizer and
UBSan and linked with the host prologue, checks on a three-box scene the rules on a request by their
messages, the launch arguments a plan fills (and that it leaves every device address null), the
tables it names for staging with their order, element sizes and counts, the cuts of a chunked frame
against brute force, the launches of plain, chunked, culled, flagged, positioned and speculative
calls in order, the classification key, and that a cached prologue keeps its march items."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_frame_launch_logic():
    subprocess.run(["make", "-C", CXX, "frame_launch_test"], check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(CXX, "frame_launch_test")], capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
