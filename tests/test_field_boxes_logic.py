"""CPU test of the box rules shared by the cell-scan products (csrc/avr_field_boxes.h: slice
images, the joint histogram, on-axis projections, derived fields) and of the 4 x 4 x 128 tile count
against its decode (csrc/avr_cell_tiles.h); no GPU call in either.  tests/cxx/field_boxes_test.cpp,
built with AddressSanitizer and UBSan, checks every refusal message and which one wins when a box
breaks two rules, `paired` per field, empty boxes, the span limit at 2^28, the tile prefix at 2^31,
and that the decode of [0, cell_tiles) visits every tile of a box exactly once."""
import os
import subprocess

CXX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cxx")


def test_field_boxes_logic():
    subprocess.run(["make", "-C", CXX, "field_boxes_test"], check=True, stdout=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(CXX, "field_boxes_test")], capture_output=True, text=True,
                         timeout=60)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
