"""Inputs of the tests that run the kernels at the two 32-bit limits the host admits, plain
Python and numpy only.  test_wide_view_cases.py holds every claim made here on the CPU;
test_wide_views_gpu.py runs the kernels on the cases.

Part A, the span rule (field_view in avr_field_boxes.h): a box may span up to 2^28 - 1 elements from
its first cell, so the byte offset of its last cell is at most 2^31 - 8.  A View is (offset into a
storage, (nx, ny, nz), jstride, kstride) in float64 elements.  A storage is one flat array of
STORAGE elements that holds POISON everywhere but in the views' cells; it exists on the device
only.  Field f of a case is the case's view moved up by f * field_shift elements, so the fields of
a multi-field product are disjoint views of one storage.

Part B, the index rule (box_index_region in avr_field_plans.h): a box's index range, refined to the
finest level, may lie anywhere in [-2^30, 2^30).  far_hierarchies() are three-level hierarchies
built as gradient_reference.make_levels builds them, and translations() shift level l by T_l with
T_(l+1) = T_l * ratio_l, so that nesting is kept exactly."""
import struct
from collections import namedtuple

import numpy as np

import gradient_reference

SEED = 2828
STORAGE = 2 ** 28 + 2 ** 20      # elements of one storage: about 2 GiB of float64
BASE = 2 ** 19                   # offset of a view with a 16-byte aligned first cell
SPAN_LIMIT = 2 ** 28 - 1         # field_view: span < 2^28
BRICK = 4                        # kBrickY = kBrickZ
CHUNK = 128                      # kClassifyChunk
MAX_FIELDS = 6                   # derive.MAX_FIELDS
WHOLE = 5                        # the field of integers: sums of its cells are exact in any order

# Finite, negative and far below every cell: read as a cell it becomes the minimum of the
# statistics, bin 0 of a histogram and table index 0 of the classify pass; written over, the
# storage no longer holds this bit pattern everywhere.
POISON = -1.2345678e300
POISON_BITS = struct.unpack("<q", struct.pack("<d", POISON))[0]

View = namedtuple("View", "offset dims jstride kstride")
Case = namedtuple("Case", "name view field_shift at_limit classify_pairs others_pair reaches")


def span(view):
    nx, ny, nz = view.dims
    return (nx - 1) + (ny - 1) * view.jstride + (nz - 1) * view.kstride


def elements(view):
    """The storage elements of the view's cells, as a set of Python integers."""
    nx, ny, nz = view.dims
    return {view.offset + i + j * view.jstride + k * view.kstride
            for k in range(nz) for j in range(ny) for i in range(nx)}


def is_paired(view):
    """FieldView::paired and for_each_cell's pair test, for a storage that starts on a 16-byte
    boundary: the first cell 16-byte aligned and both strides even."""
    return view.offset % 2 == 0 and view.jstride % 2 == 0 and view.kstride % 2 == 0


def classify_is_paired(view):
    """classify_tile's pair test: the same, and the row stride below 2^27."""
    return is_paired(view) and view.jstride < 2 ** 27


def field_view(case, field):
    return case.view._replace(offset=case.view.offset + field * case.field_shift)


def _case(name, offset, dims, jstride, kstride, reaches, field_shift=8):
    view = View(offset, dims, jstride, kstride)
    return Case(name, view, field_shift, span(view) == SPAN_LIMIT, classify_is_paired(view),
                is_paired(view), reaches)


def wide_cases():
    """Cases 1 to 5 of the span rule.  The js = 2^27 - 2 twin of case 3 has two cells per row and
    kstride = 2^27: at the span limit with two rows and two planes, kstride = 2^28 - nx - jstride,
    and rows of more than two cells would then run into the row 2^27 - 2 elements on."""
    return [
        _case("end_pair", BASE, (6, 2, 2), 2 ** 26, 2 ** 28 - 2 ** 26 - 6,
              "pair path everywhere; the last pair ends at byte 2^31 of the view"),
        _case("odd_row_end", BASE, (5, 2, 2), 2 ** 26, 2 ** 28 - 2 ** 26 - 6,
              "the last cell of every row is the pair path's single-cell tail"),
        # plane 1 begins eight elements below row 1: fields 16 apart keep their rows of seven apart
        _case("row_stride_at_cap", BASE, (7, 2, 2), 2 ** 27, 2 ** 27 - 8,
              "classify unpaired (jstride = 2^27), statistics and FieldView::paired pair", 16),
        _case("row_stride_below_cap", BASE, (2, 2, 2), 2 ** 27 - 2, 2 ** 27,
              "the last jstride classify pairs, at the span limit"),
        _case("unpaired_at_limit", BASE + 1, (6, 2, 2), 2 ** 26 + 1, 2 ** 28 - 2 ** 26 - 7,
              "single cells: base 8 mod 16, odd strides, the largest odd kstride"),
        # rows of 130 cells 132 apart: a field's rows fill its plane, so the next field starts
        # eight rows up
        _case("chunk_crossing_paired", BASE, (130, 5, 2), 132, 2 ** 28 - 658,
              "a row crosses the 128-cell chunk, the second brick of rows is partial", 8 * 132),
        _case("chunk_crossing_unpaired", BASE + 1, (130, 5, 2), 132, 2 ** 28 - 659,
              "the same with single cells", 8 * 132),
    ]


# ---- cells -------------------------------------------------------------------------------------

def field_cells(case, field, odd=False):
    """[nz, ny, nx] float64: distinct values in (1 + field, 2 + field), so that no two cells of a
    case's fields are equal; the box's last cell holds the largest and the cell before it the
    second largest, so that zeros or poison in their place move a maximum.  odd: cells 1, 2 and 3
    of the first row are NaN, +Inf and -Inf.  Field WHOLE holds distinct integers instead, from
    1000 on: the products that add cells up with atomics give its sums bit for bit in any order."""
    nx, ny, nz = case.view.dims
    n = nx * ny * nz
    rng = np.random.default_rng([SEED, field, n])
    if field == WHOLE:
        return (1000.0 + rng.permutation(n)).reshape(nz, ny, nx)
    flat = 1.0 + field + (rng.permutation(n - 2) + 0.5) / n
    flat = np.concatenate([flat, [1.0 + field + (n - 1.5) / n, 1.0 + field + (n - 0.5) / n]])
    if odd:
        flat[1:4] = [np.nan, np.inf, -np.inf]
    return flat.reshape(nz, ny, nx)


def small_cells(dims, tag):
    """The cells of an ordinary contiguous box: distinct values in (8 + tag, 9 + tag); distinct
    integers from 10000 * (1 + tag) on where tag % 10 is WHOLE."""
    nx, ny, nz = dims
    n = nx * ny * nz
    rng = np.random.default_rng([SEED, 100 + tag, n])
    if tag % 10 == WHOLE:
        return (10000.0 * (1 + tag) + rng.permutation(n)).reshape(nz, ny, nx)
    return (8.0 + tag + (rng.permutation(n) + 0.5) / n).reshape(nz, ny, nx)


# ---- the scenes around a wide box -----------------------------------------------------------------

CELL = 0.125                     # level-0 cell size on every axis; level 1 halves it
RATIO = [2]
PLAIN_NX = 4
FINE_DIMS = (4, 2, 2)

SceneBox = namedtuple("SceneBox", "kind level index_lo dims")


def hierarchy(case, wide_first=True):
    """The two-level scene of a case: the wide box at index (0, 0, 0) of level 0, an ordinary box
    of 4 x ny x nz cells beside it along x, and one level-1 box of 4 x 2 x 2 cells over the last
    cell of the wide box's first row and the first of the ordinary box's.  The wide box's last
    cell (nx - 1, ny - 1, nz - 1) stays a leaf."""
    nx, ny, nz = case.view.dims
    wide = SceneBox("wide", 0, (0, 0, 0), (nx, ny, nz))
    plain = SceneBox("plain", 0, (nx, 0, 0), (PLAIN_NX, ny, nz))
    fine = SceneBox("fine", 1, (2 * (nx - 1), 0, 0), FINE_DIMS)
    return [wide, plain, fine] if wide_first else [plain, wide, fine]


def level_sizes():
    return [(CELL,) * 3, (CELL / 2,) * 3]


def corners(box):
    size = CELL / 2 ** box.level
    return (tuple(lo * size for lo in box.index_lo),
            tuple((lo + n) * size for lo, n in zip(box.index_lo, box.dims)))


def extent(case):
    """The physical size of the scene (prob_lo is the origin)."""
    nx, ny, nz = case.view.dims
    return ((nx + PLAIN_NX) * CELL, ny * CELL, nz * CELL)


# ---- part B: far index origins --------------------------------------------------------------------

INDEX_LIMIT = 2 ** 30

Hierarchy = namedtuple("Hierarchy", "name ratio domains boxes")


def far_hierarchies():
    return [
        Hierarchy("ratios_2_2", [2, 2],
                  [((0, 0, 0), (5, 3, 3)), ((0, 0, 0), (11, 7, 7)), ((0, 0, 0), (23, 15, 15))],
                  [[((0, 0, 0), (2, 3, 3)), ((3, 0, 0), (5, 3, 3))],
                   [((2, 2, 2), (5, 5, 5)), ((6, 2, 2), (9, 7, 5))],
                   [((6, 6, 6), (9, 9, 9))]]),
        Hierarchy("ratios_4_2", [4, 2],
                  [((0, 0, 0), (5, 3, 3)), ((0, 0, 0), (23, 15, 15)), ((0, 0, 0), (47, 31, 31))],
                  [[((0, 0, 0), (5, 3, 3))],
                   [((8, 4, 4), (15, 11, 11))],
                   [((20, 12, 12), (27, 19, 19))]]),
    ]


def translations(h):
    """{"top": T, "bottom": T}, T[l] = (tx, ty, tz) of level l: the level-0 domain refined to the
    finest level ends at index 2^30 - 1 on every axis, or begins at -2^30."""
    refine = h.ratio[0] * h.ratio[1]
    lo, hi = h.domains[0]
    out = {}
    for name in ("top", "bottom"):
        if name == "top":
            t0 = tuple((INDEX_LIMIT - (hi[a] + 1) * refine) // refine for a in range(3))
        else:
            t0 = tuple((-INDEX_LIMIT - lo[a] * refine) // refine for a in range(3))
        t1 = tuple(t * h.ratio[0] for t in t0)
        out[name] = [t0, t1, tuple(t * h.ratio[1] for t in t1)]
    return out


def shifted(region, t):
    lo, hi = region
    return (tuple(lo[a] + t[a] for a in range(3)), tuple(hi[a] + t[a] for a in range(3)))


def far_levels(h, translation=None):
    """gradient_reference.make_levels of the hierarchy (the same cells whatever the translation),
    with every domain and box moved by the translation's T_l."""
    levels = gradient_reference.make_levels(h.domains, h.boxes, h.ratio, SEED)
    if translation is None:
        return levels
    return [{"domain": shifted(lev["domain"], t), "boxes": [shifted(b, t) for b in lev["boxes"]],
             "data": lev["data"]} for lev, t in zip(levels, translation)]
