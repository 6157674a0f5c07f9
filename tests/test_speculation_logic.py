"""CPU test of the frame driver's visibility speculation (csrc/avr_speculation.h, no GPU call in
it): tests/cxx/speculation_test.cpp feeds the state machine what the driver feeds it -- frames,
arrived observations, repairs -- with 8 local boxes: activation and rejection, the saving floor,
the memory of 24 frames, an emptied set, observations kept by box across plans, the back-off on
repairs in more than half of 32 frames and its doubling sleeps, the deciding state, forget(), and
which active frames are observed."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_speculation_logic():
    subprocess.run(["make", "-C", CXX, "speculation_test"], check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(CXX, "speculation_test")], capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
