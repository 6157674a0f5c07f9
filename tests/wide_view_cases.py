"""Inputs of the tests that run the kernels at the two 32-bit limits the host admits, plain
Python and numpy only.  test_wide_view_cases.py holds every claim made here on the CPU;
test_wide_views_gpu.py and test_far_index_origins_gpu.py run the kernels on the cases.

Part A, the span rule (field_view in avr_field_boxes.h): a box may span up to 2^28 - 1 elements from
its first cell, so the byte offset of its last cell is at most 2^31 - 8.  A View is (offset into a
storage, (nx, ny, nz), jstride, kstride) in float64 elements.  A storage is one flat array of
STORAGE elements that holds POISON everywhere but in the views' cells; it exists on the device
only.  Field f of a case is the case's view moved up by f * field_shift elements, so the fields of
a multi-field product are disjoint views of one storage.

Part B, the index rule (box_index_region in avr_field_plans.h): a box's index range, refined to the
finest level, may lie anywhere in [-2^30, 2^30).  far_hierarchies() are three-level hierarchies
built as gradient_reference.make_levels builds them, and translations() shift level l by T_l with
T_(l+1) = T_l * ratio_l, so that nesting is kept exactly.

The inputs of the products that came after the two modules (grid fields, velocity cubes, ray
transfer, particle fields, clump binding) are here too, so that the GPU tests and the CPU claims
share them: scene_levels() gives a wide scene to the numpy references, wide_particles(),
wide_grids() and the channel edges are part A's, far_particles(), far_fields() and the far edges
part B's."""
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


def scene_levels(case, fields=(0,)):
    """The case's scene as the numpy references take a plotfile's levels (levels[l] = {"domain",
    "boxes", "data": [array [len(fields), nz, ny, nx]]}): the wide and the plain box are the grids
    of level 0, the fine box the grid of level 1.  Field 0 has its NaN and infinities, as the GPU
    tests install it."""
    nx, ny, nz = case.view.dims
    by_kind = {b.kind: b for b in hierarchy(case)}

    def region(b):
        return (b.index_lo, tuple(lo + n - 1 for lo, n in zip(b.index_lo, b.dims)))

    def data(kind, tag):
        return np.stack([field_cells(case, f, odd=(f == 0)) if kind == "wide"
                         else small_cells(by_kind[kind].dims, tag + f) for f in fields])

    whole = (nx + PLAIN_NX, ny, nz)
    return [{"domain": ((0, 0, 0), tuple(n - 1 for n in whole)),
             "boxes": [region(by_kind["wide"]), region(by_kind["plain"])],
             "data": [data("wide", 0), data("plain", 0)]},
            {"domain": ((0, 0, 0), tuple(2 * n - 1 for n in whole)),
             "boxes": [region(by_kind["fine"])], "data": [data("fine", 10)]}]


# ---- part A: the inputs of the newer products --------------------------------------------------

# Velocity cubes bin field 1, which lies in (2, 3) in the wide box, (9, 10) in the plain box and
# (19, 20) in the fine one: five channels with wide cells under the first edge, the wide box's last
# two cells in the last channel and every other box over.
CUBE_EDGES = np.linspace(2.2, 3.0, 6)
# Ray transfer bins field 3, (4, 5) in the wide box: three channels, the other boxes over.
TRANSFER_EDGES = np.array([4.25, 4.5, 4.75, 5.0])
# The opacity is field 2 times a power of two (exact, and exactly undone): a ray along the 130
# cells of the longest row then has an optical depth of 16.25 * 3.5 / 16, about 3.5.
OPACITY_SCALE = 2.0 ** -4
CLUMP_LOWER, CLUMP_UPPER = 1.4, 30.0         # of field 0: the wide box's last cell is a member
N_FIXED = 5                                  # the particles placed by hand come first


def empty_cell(case):
    """The cell of the wide box that no particle's cell or cloud names."""
    _, ny, nz = case.view.dims
    return (0, ny - 1, nz - 1)


def wide_particles(case):
    """(points [n, 3], values [n]) of a case's scene, n about 300, more than one workgroup of 256.
    Rows 0 to 4 are placed by hand: in the wide box's first cell; at three quarters of its last
    cell on every axis, so that its cloud leaves the domain in y and z and reaches the plain box in
    x; on the face between the wide and the plain box, in the last row; two inside the fine box.
    The others are uniform over the scene and a tenth of it beyond each side, without those within
    one level-0 cell of the centre of empty_cell(case) on every axis: no cloud reaches that cell."""
    nx, ny, nz = case.view.dims
    rng = np.random.default_rng([SEED, 40, nx * ny * nz])
    points = rng.uniform(-0.1, 1.1, (360, 3)) * np.array(extent(case))
    centre = (np.array(empty_cell(case)) + 0.5) * CELL
    points = points[(np.abs(points - centre[None, :]) > CELL).any(axis=1)]
    fixed = np.array([(0.25, 0.25, 0.25),
                      (nx - 0.25, ny - 0.25, nz - 0.25),
                      (nx, ny - 0.75, nz - 0.75),
                      (nx - 0.7, 0.3, 0.6),
                      (nx + 0.55, 0.7, 0.2)]) * CELL
    assert len(fixed) == N_FIXED
    points = np.concatenate([fixed, points])
    values = rng.standard_normal(len(points))
    values[:N_FIXED] = [1.5, 2.5, -3.5, 4.5, 5.5]
    return points, values


def _grid(dims, tag):
    """[nz, ny, nx]: distinct finite values in (-0.5, 0.5) and one NaN in the middle."""
    n = dims[0] * dims[1] * dims[2]
    flat = (np.random.default_rng([SEED, 50 + tag, n]).permutation(n) + 0.5) / n - 0.5
    flat[n // 2] = np.nan
    return flat.reshape(dims[::-1])


WideGrid = namedtuple("WideGrid", "name level lo grid modes")


def wide_grids(case):
    """The uniform grids written onto a case's scene; modes are (interpolation, periodic).
    margin: level 0 over the domain and one cell beyond it on -x, the same level for the level-0
    boxes and the coarser one for the fine box.  refined: level 1 over the whole domain, the finer
    one for the level-0 boxes.  partial: level 1 from (3, 1, 1) to the wide box's high x and y faces
    and two cells thick in z, so that column 0 of the wide box gets fill and every other cell of
    it, its last one included, is covered in part."""
    nx, ny, nz = case.view.dims
    whole = (nx + PLAIN_NX, ny, nz)
    return [WideGrid("margin", 0, (-1, 0, 0), _grid((whole[0] + 1, ny, nz), 0),
                     [(0, False), (1, False), (1, True)]),
            WideGrid("refined", 1, (0, 0, 0), _grid(tuple(2 * n for n in whole), 1), [(0, False)]),
            WideGrid("partial", 1, (3, 1, 1), _grid((2 * nx - 3, 2 * ny - 1, 2), 2), [(0, False)])]


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


# ---- part B: the inputs of the newer products --------------------------------------------------

FAR_SIZE_0 = 0.25                # a power of two; the finer levels divide it by their ratios
FAR_PROB_LO = (0.0, -1.0, 2.0)   # of the untranslated hierarchy


def far_geometry(h, translation=None):
    """(cell sizes per level, prob_lo') at a translation: prob_lo' = prob_lo - T_0 * size_0, exact,
    so that the physical domain is where FAR_PROB_LO puts it, whatever the translation."""
    t0 = translation[0] if translation is not None else (0, 0, 0)
    refine = [1, h.ratio[0], h.ratio[0] * h.ratio[1]]
    return ([(FAR_SIZE_0 / r,) * 3 for r in refine],
            tuple(FAR_PROB_LO[a] - t0[a] * FAR_SIZE_0 for a in range(3)))


def far_extent(h):
    lo, hi = h.domains[0]
    return np.array([(hi[a] - lo[a] + 1) * FAR_SIZE_0 for a in range(3)])


def far_points(h, n, seed):
    """n points of the physical domain, a tenth of it beyond each side included."""
    rng = np.random.default_rng([SEED, seed])
    return np.array(FAR_PROB_LO) + rng.uniform(-0.1, 1.1, (n, 3)) * far_extent(h)


FarParticles = namedtuple("FarParticles", "points values lattice")


def far_particles(h):
    """The particles of a hierarchy; lattice is the slice of those on multiples of 1/64, whose
    positions relative to prob_lo' are exact under every translation.  Uniform points; the lattice
    batch; points inside the finest box and inside each level-1 box; the two domain corners
    themselves; and points an eighth of a finest cell inside the bottom and the top face of the
    domain on one, two and three axes, whose clouds reach one cell past the domain."""
    rng = np.random.default_rng([SEED, 60, len(h.boxes[1])])
    low, size = np.array(FAR_PROB_LO), far_extent(h)
    sizes, _ = far_geometry(h)
    uniform = far_points(h, 192, 11)
    steps = np.rint(size * 64).astype(np.int64)
    lattice = low + np.stack([rng.integers(-s // 10, s + s // 10 + 1, 128) for s in steps],
                             axis=1) / 64.0
    inside = []
    for level, count in ((2, 48), (1, 40)):
        for lo, hi in h.boxes[level]:
            span_ = np.array(hi) - np.array(lo) + 1
            inside.append(low + (np.array(lo) + rng.random((count, 3)) * span_) * sizes[level][0])
    eighth = sizes[2][0] / 8.0
    faces = []
    for axes in ((0,), (1,), (2,), (0, 1), (0, 1, 2)):
        for top in (False, True):
            p = low + rng.uniform(0.2, 0.8, 3) * size
            for a in axes:
                p[a] = low[a] + size[a] - eighth if top else low[a] + eighth
            faces.append(p)
    points = np.concatenate([uniform, lattice] + inside + [np.stack([low, low + size]),
                                                           np.stack(faces)])
    return FarParticles(points, rng.standard_normal(len(points)), slice(192, 192 + 128))


def rerouted_corners(hier, points):
    """The cloud-in-cell corners of `points` that no leaf of `hier` (a particle_reference
    hierarchy) holds, from q alone: [(leaf level, corner index [3] in that level)]."""
    level, q, _ = hier.locate(np.ascontiguousarray(points, dtype=np.float64))
    out = []
    for l in range(hier.max_level + 1):
        pick = np.nonzero(level == l)[0]
        if not pick.size:
            continue
        base = np.floor(q[pick] - 0.5).astype(np.int64)
        for c in range(8):
            index = base + np.array([c & 1, (c >> 1) & 1, c >> 2], dtype=np.int64)[None, :]
            present = hier.corner(l, index)[0]
            out += [(l, tuple(int(v) for v in row)) for row in index[~present]]
    return out


def finest_range(h, level, index):
    """The first and the last finest-level index under index `index` of `level`, one axis."""
    r = [h.ratio[0] * h.ratio[1], h.ratio[1], 1][level]
    return index * r, (index + 1) * r - 1


# The stored components are u, odd, whole (gradient_reference.VARIABLES); data is [3, nz, ny, nx].
FAR_FIELDS = {
    "source": lambda data: data[0].copy(),
    "opacity": lambda data: np.abs(data[2]) * 2.0 ** -10,       # optical depths of order 1
    "bin": lambda data: data[2] * 0.5,                          # a half-integer lattice
    "width": lambda data: np.minimum(0.1 + np.abs(data[0]) * 10.0, 30.0) * 31.25,
}
FAR_SHARP_EDGES = np.array([-400.0, -100.0, 150.0, 420.0])      # some of bin under, some over
FAR_BROAD_EDGES = np.array([-46.875, -15.625, 15.625, 46.875])  # channels 31.25 wide


def far_field_levels(levels, name):
    """The levels with the one component FAR_FIELDS[name] gives, for ray_reference.Hierarchy."""
    return [{"domain": lev["domain"], "boxes": lev["boxes"],
             "data": [FAR_FIELDS[name](data)[None] for data in lev["data"]]} for lev in levels]


def far_grid(dims, seed):
    return np.random.default_rng([SEED, 70, seed]).standard_normal(tuple(dims)[::-1])
