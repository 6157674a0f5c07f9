"""Clumps on the GPU: the kernels of avr_clumps.hip through avr_scene_clumps and
avr_scene_clump_table, api.clump_scene, api.clumps and the registry, against the numpy reference on
the plotfile's own level arrays (clump_reference).  Label fields are equal by bits; counts are
equal; a sum lies within (n - 1) 2^-53 sum |vs| of the correctly rounded one (plus that one's own
rounding), the a-priori bound of n f64 additions in any order.  Cell sizes are powers of two, and
every coarse cell that a finer grid covers holds 1e30: with upper = +inf a read of a parent grid
past a leaf box's view would show as a wrong clump."""
import ctypes as C
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, plotfile
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform

import clump_reference as cr
import gradient_reference as ref

pytestmark = pytest.mark.gpu
VARIABLES = list(ref.VARIABLES)
INF = math.inf
U = 2.0 ** -53


@pytest.fixture(autouse=True)
def _empty_registries():
    def clear():
        for name in list(api.clump_fields()):
            api.remove_clump_field(name)
        for name in list(api.gradient_fields()):
            api.remove_gradient_field(name)
        for name in list(api.derived_fields()):
            api.remove_field(name)
    clear()
    yield
    clear()


@dataclasses.dataclass(eq=False)
class Case:
    path: str
    levels: list
    lo: tuple
    hi: tuple
    ratio: list
    names: list

    def sizes(self):
        return ref.cell_sizes(self.levels, self.lo, self.hi)

    def scene_boxes(self, min_level=0, max_level=-1):
        """(level, lo, hi) of every scene box, in the loader's order."""
        if max_level < 0:
            max_level = len(self.levels) - 1
        convex = plotfile.convexify([lev["boxes"] for lev in self.levels[:max_level + 1]],
                                    self.ratio[:max_level])
        return [(l, lo, hi) for l in range(min_level, max_level + 1) for _, (lo, hi) in convex[l]]

    @functools.lru_cache(maxsize=None)
    def reference(self, variable, lower, upper, min_level=0, max_level=-1):
        return cr.clump_levels(self.levels, self.ratio, self.names.index(variable), lower, upper,
                               self.scene_boxes(min_level, max_level), min_level, max_level)

    def leaves(self, variable, min_level=0, max_level=-1):
        return ref.leaf_arrays(self.levels, self.ratio, self.names.index(variable), min_level,
                               max_level)[0]

    def cut(self, dense, level, lo, hi):
        dlo = self.levels[level]["domain"][0]
        return dense[level][lo[2] - dlo[2]:hi[2] - dlo[2] + 1, lo[1] - dlo[1]:hi[1] - dlo[1] + 1,
                            lo[0] - dlo[0]:hi[0] - dlo[0] + 1]


def _write(path, domains, boxes, lo, hi, ratio, seed, extra=None):
    levels = ref.make_levels(domains, boxes, ratio, seed)
    case = Case(str(path), levels, lo, hi, list(ratio), list(VARIABLES))
    for size in case.sizes():
        assert all(np.frexp(s)[0] == 0.5 for s in size)             # powers of two
    written = levels
    if extra is not None:
        more = extra(case)
        case.names = VARIABLES + list(more)
        written = [{"domain": lev["domain"], "boxes": lev["boxes"],
                    "data": [np.concatenate([data] + [case.cut(dense, l, *box)[None]
                                                      for dense in more.values()])
                             for box, data in zip(lev["boxes"], lev["data"])]}
                   for l, lev in enumerate(levels)]
        case.levels = written
    plotfile.write_plotfile(str(path), case.names, written, lo, hi, ratio)
    return case


def _write_fields(path, grids, domain, hi, fields):
    """One level whose fields are given over the domain: fields[name] = array [nz, ny, nx]."""
    names = list(fields)
    data = [np.stack([fields[n][lo[2]:bhi[2] + 1, lo[1]:bhi[1] + 1, lo[0]:bhi[0] + 1]
                      for n in names]) for lo, bhi in grids]
    levels = [{"domain": domain, "boxes": list(grids), "data": data}]
    case = Case(str(path), levels, (0.0, 0.0, 0.0), hi, [], names)
    plotfile.write_plotfile(str(path), names, levels, case.lo, hi, [])
    return case


THREE_DOMAINS = [((0, 0, 0), (11, 5, 7)), ((0, 0, 0), (23, 11, 15)), ((0, 0, 0), (47, 23, 31))]
# two fine boxes that touch at i = 11 | 12; the finest grid lies inside the first
THREE_BOXES = [[((0, 0, 0), (6, 5, 7)), ((7, 0, 0), (11, 5, 7))],
               [((4, 2, 2), (11, 7, 9)), ((12, 2, 2), (17, 9, 9))],
               [((12, 6, 6), (21, 13, 15))]]
BROAD = (-0.5, INF)        # about 69 % of a normal field: one clump through every level, and others


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    """Three levels at ratio 2, non-cubic; stored next to the fields: the reference's labels of u
    over BROAD, so that products of the clump field have a stored twin."""
    twins = lambda case: {"clump_stored": case.reference("u", *BROAD)[0]}
    return _write(tmp_path_factory.mktemp("clumps") / "three", THREE_DOMAINS, THREE_BOXES,
                  (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 2], 41, twins)


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    grids = [((0, 0, 0), (130, 4, 2)), ((131, 0, 0), (386, 3, 3)), ((387, 0, 0), (387, 3, 3)),
             ((388, 0, 0), (390, 3, 3)), ((395, 7, 7), (395, 7, 7))]
    return _write(tmp_path_factory.mktemp("clumps") / "shapes", [((0, 0, 0), (399, 7, 7))],
                  [grids], (0.0, 0.0, 0.0), (100.0, 2.0, 2.0), [], 42)


@pytest.fixture(scope="module")
def ratio_four(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("clumps") / "four",
                  [((0, 0, 0), (5, 3, 3)), ((0, 0, 0), (23, 15, 15))],
                  [[((0, 0, 0), (5, 3, 3))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (3.0, 2.0, 2.0), [4], 43)


@pytest.fixture(scope="module")
def skipped_level(tmp_path_factory):
    """The finest grid covers the low-x half of the middle one: a level-0 leaf lies face to face
    with level-2 cells."""
    return _write(tmp_path_factory.mktemp("clumps") / "skipped",
                  [((0, 0, 0), (7, 3, 3)), ((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))],
                  [[((0, 0, 0), (7, 3, 3))], [((4, 2, 2), (11, 5, 5))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [2, 2], 44)


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    grids = [((4 * a, 4 * b, 4 * c), (4 * a + 3, 4 * b + 3, 4 * c + 3))
             for c in range(5) for b in range(4) for a in range(4)]
    return _write(tmp_path_factory.mktemp("clumps") / "many", [((0, 0, 0), (15, 15, 19))],
                  [grids], (0.0, 0.0, 0.0), (2.0, 2.0, 2.5), [], 45)


def load(ctx, case, name, min_level=0, max_level=-1):
    return plotfile.load_plotfile_geometry(ctx, case.path, name, min_level, max_level, False, True)


def clumps_of(ctx, case, variable, lower, upper, min_level=0, max_level=-1):
    scene = load(ctx, case, variable, min_level, max_level)
    finest = max(b.level for b in scene.all_boxes)
    out, n = api.clump_scene(ctx, scene, lower, upper, case.sizes()[:finest + 1], case.lo,
                             case.ratio)
    ctx.synchronize()
    return out, n, scene


def check(ctx, case, variable, lower, upper, min_level=0, max_level=-1):
    out, n, scene = clumps_of(ctx, case, variable, lower, upper, min_level, max_level)
    dense, count = case.reference(variable, lower, upper, min_level, max_level)
    expected = case.scene_boxes(min_level, max_level)
    assert len(out.local_boxes) == len(out.all_boxes) == len(expected) > 0
    assert out.world_scale == scene.world_scale
    for box, (level, lo, hi) in zip(out.local_boxes, expected):
        assert box.level == level
        assert box.cell_dimensions == tuple(hi[a] - lo[a] + 1 for a in range(3))
        assert ref.same_bits(box.values.cpu().numpy(), case.cut(dense, level, lo, hi)), \
            (variable, lower, upper, level, lo, hi)
    assert n == count
    return out, n, scene


def pair_path(scene):
    even = lambda b: (b.values.data_ptr() % 16 == 0 and b.values.stride(1) % 2 == 0 and
                      b.values.stride(0) % 2 == 0)
    return [even(b) for b in scene.local_boxes]


# ---- hierarchy -----------------------------------------------------------------------------------

def test_three_levels_with_clumps_through_every_kind_of_face(ctx, three):
    _, n, scene = check(ctx, three, "u", *BROAD)
    paths = pair_path(scene)
    assert any(paths) and not all(paths)          # leaf boxes are odd-strided views of their grids
    # what the threshold gives, by the reference: several clumps, fine-to-coarse links along every
    # axis and from either side, and one clump in both level-1 grids
    arrays = three.leaves("u")
    selected = cr.selected_arrays(arrays, *BROAD)
    crossing = {(axis, step) for a, b, axis, step in cr.adjacent_pairs(arrays, selected, [2, 2])
                if a[0] != b[0]}
    assert crossing == {(a, s) for a in range(3) for s in (-1, 1)}
    dense = three.reference("u", *BROAD)[0]
    first, second = (set(three.cut(dense, 1, *box).ravel().tolist()) - {0.0}
                     for box in THREE_BOXES[1])
    assert first & second and n > 3
    _, sparse, _ = check(ctx, three, "u", 0.4, INF)      # about a third: many clumps
    assert sparse > 20
    check(ctx, three, "u", -INF, INF)                    # everything, the 1e30 cells would join


def test_ratio_four(ctx, ratio_four):
    check(ctx, ratio_four, "u", *BROAD)
    check(ctx, ratio_four, "u", 0.3, INF)


def test_a_coarse_leaf_face_to_face_with_cells_two_levels_finer(ctx, skipped_level):
    arrays = skipped_level.leaves("u")
    assert arrays[0][1][1, 1, 1] and not arrays[0][1][1, 1, 2] and not arrays[1][1][2, 2, 4]
    selected = cr.selected_arrays(arrays, -INF, INF)
    assert any(a[0] == 2 and b[0] == 0
               for a, b, _, _ in cr.adjacent_pairs(arrays, selected, [2, 2]))
    check(ctx, skipped_level, "u", *BROAD)
    check(ctx, skipped_level, "u", 0.2, INF)
    assert check(ctx, skipped_level, "u", -INF, INF)[1] == 1


@pytest.mark.parametrize("levels", [(1, -1), (0, 0)])
def test_level_ranges_leave_holes_and_whole_coarse_grids(ctx, three, levels):
    check(ctx, three, "u", *BROAD, *levels)
    check(ctx, three, "u", 0.4, INF, *levels)


def test_eighty_boxes(ctx, many):
    out, n, _ = check(ctx, many, "u", 0.3, INF)
    assert len(out.local_boxes) == 80 and n > 10
    assert check(ctx, many, "u", -INF, INF)[1] == 1


# ---- shapes --------------------------------------------------------------------------------------

def test_rows_of_131_and_256_cells_a_thin_box_and_a_lone_cell(ctx, shapes):
    out, n, scene = check(ctx, shapes, "u", *BROAD)
    assert pair_path(scene) == [False, True, False, False, False]
    assert [b.cell_dimensions for b in out.local_boxes] == [(131, 5, 3), (256, 4, 4), (1, 4, 4),
                                                            (3, 4, 4), (1, 1, 1)]
    check(ctx, shapes, "u", 0.3, INF)
    out, n, _ = check(ctx, shapes, "u", -INF, INF)
    assert n == 2 and out.local_boxes[4].values.cpu().numpy().tolist() == [[[2.0]]]


@pytest.fixture(scope="module")
def serpentine(tmp_path_factory):
    """64 x 16 x 4: in planes 0 and 2 a path one cell wide that runs along x in every second row,
    the rows joined at alternating ends; planes 1 and 3 hold one cell each, which joins the path
    of the plane below to what lies above it; everything else is 0."""
    field = np.zeros((4, 16, 64))
    for k in (0, 2):
        for n, j in enumerate(range(0, 16, 2)):
            field[k, j, :] = 1.0
            if j + 2 < 16:
                field[k, j + 1, 63 if n % 2 == 0 else 0] = 1.0
    field[1, 14, 0] = 1.0
    field[3, 0, 0] = 1.0
    return _write_fields(tmp_path_factory.mktemp("clumps") / "snake", [((0, 0, 0), (63, 15, 3))],
                         ((0, 0, 0), (63, 15, 3)), (64.0, 16.0, 4.0), {"path": field})


def test_one_clump_that_snakes_through_a_box(ctx, serpentine):
    out, n, _ = check(ctx, serpentine, "path", 0.5, 1.5)
    labels = out.local_boxes[0].values.cpu().numpy()
    assert n == 1 and int((labels == 1.0).sum()) > 1000


# ---- numbering -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def checkerboard(tmp_path_factory):
    k, j, i = np.indices((64, 128, 128))
    field = ((i + j + k) % 2).astype(np.float64)
    grids = [((64 * a, 64 * b, 0), (64 * a + 63, 64 * b + 63, 63)) for b in range(2)
             for a in range(2)]
    return _write_fields(tmp_path_factory.mktemp("clumps") / "checker", grids,
                         ((0, 0, 0), (127, 127, 63)), (128.0, 128.0, 64.0), {"parity": field})


def test_a_checkerboard_numbers_every_selected_cell_in_ordinal_order(ctx, checkerboard):
    out, n, _ = clumps_of(ctx, checkerboard, "parity", 0.5, INF)
    assert n == 2 ** 19
    begin = 0
    for box, (level, lo, hi) in zip(out.local_boxes, checkerboard.scene_boxes()):
        want = checkerboard.cut([_domain_field(checkerboard)], 0, lo, hi)
        flat = want.reshape(-1)
        labels = np.where(flat > 0.5, begin + np.cumsum(flat > 0.5), 0).astype(np.float64)
        assert ref.same_bits(box.values.cpu().numpy().reshape(-1), labels)
        begin += int((flat > 0.5).sum())
    assert begin == n
    # everything selected is one clump, nothing selected none
    out, n, _ = clumps_of(ctx, checkerboard, "parity", -INF, INF)
    assert n == 1 and all(bool((b.values == 1.0).all()) for b in out.local_boxes)
    out, n, _ = clumps_of(ctx, checkerboard, "parity", 2.0, 3.0)
    assert n == 0
    assert all(ref.same_bits(b.values.cpu().numpy(), np.zeros(tuple(b.values.shape)))
               for b in out.local_boxes)


def _domain_field(case):
    (dlo, dhi) = case.levels[0]["domain"]
    dense = np.zeros(tuple(dhi[a] - dlo[a] + 1 for a in (2, 1, 0)))
    for (lo, hi), data in zip(case.levels[0]["boxes"], case.levels[0]["data"]):
        dense[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = data[0]
    return dense


# ---- values --------------------------------------------------------------------------------------

def test_closed_bounds_on_an_integer_field(ctx, three):
    arrays = three.leaves("whole")
    values = np.unique(np.concatenate([v[m] for _, m, v in arrays]))
    lower, upper = float(values[len(values) // 3]), float(values[2 * len(values) // 3])
    check(ctx, three, "whole", lower, upper)     # cells exactly at either bound are selected
    check(ctx, three, "whole", lower, lower)
    selected = cr.selected_arrays(arrays, lower, lower)
    assert sum(int(s.sum()) for s in selected) >= 1


def test_nan_and_infinities(ctx, three):
    check(ctx, three, "odd", -INF, INF)          # all but the NaNs
    check(ctx, three, "odd", -0.2, INF)          # +Inf is in, -Inf is out
    check(ctx, three, "odd", -INF, 0.2)
    check(ctx, three, "odd", -1e300, 1e300)      # neither infinity


def test_a_repeat_gives_equal_bits_and_equal_n(ctx, three):
    first, n, _ = clumps_of(ctx, three, "odd", -0.3, INF)
    again, m, _ = clumps_of(ctx, three, "odd", -0.3, INF)
    assert n == m
    for a, b in zip(first.local_boxes, again.local_boxes):
        assert ref.same_bits(a.values.cpu().numpy(), b.values.cpu().numpy())


# ---- the C ABI's checks ----------------------------------------------------------------------------

def test_wrong_arguments_are_refused_and_the_outputs_untouched(ctx, three):
    f = load(ctx, three, "u")
    coarse = load(ctx, three, "u", 0, 0)
    sf = ctx.create_scene(f.local_boxes, f.scalar_transform)
    other = ctx.create_scene(coarse.local_boxes, coarse.scalar_transform)
    narrow = ctx.create_scene([dataclasses.replace(f.local_boxes[0],
                                                   values=f.local_boxes[0].values[:, :, :-1])]
                              + f.local_boxes[1:], f.scalar_transform)
    relevelled = ctx.create_scene(f.local_boxes[:-1] + [dataclasses.replace(f.local_boxes[-1],
                                                                             level=0)],
                                  f.scalar_transform)
    sentinel = 0.5
    outs = [AmrBox(b.min_corner, b.max_corner,
                   torch.full(b.values.shape, sentinel, dtype=torch.float64, device=ctx.device),
                   b.level) for b in f.local_boxes]
    out = ctx.create_scene(outs, ScalarTransform())
    count = torch.full((1,), -7, dtype=torch.int64, device=ctx.device)
    boxes = three.scene_boxes()
    index = np.array([lo for _, lo, _ in boxes], dtype=np.int32)

    def untouched():
        ctx.synchronize()
        return all(bool((b.values == sentinel).all()) for b in outs) and int(count.item()) == -7

    def call(field=sf, target=out, lower=-0.5, upper=INF, index=index, ratio=(2, 2), n_levels=3):
        index = np.ascontiguousarray(index, np.int32)
        ratio = np.ascontiguousarray(ratio, np.int32)
        return _capi.lib().avr_scene_clumps(
            ctx._handle, field._handle, target._handle, lower, upper,
            index.ctypes.data_as(C.POINTER(C.c_int32)), ratio.ctypes.data_as(C.POINTER(C.c_int32)),
            n_levels, C.c_void_p(count.data_ptr()))

    overlapping = index.copy()
    same_level = [b for b, (level, _, _) in enumerate(boxes) if level == 1]
    overlapping[same_level[1]] = index[same_level[0]]
    far = index.copy()
    far[0, 0] = 2 ** 30
    wrong = [
        dict(lower=math.nan), dict(upper=math.nan), dict(lower=1.0, upper=0.5),
        dict(lower=INF, upper=-INF),
        dict(n_levels=0), dict(n_levels=17, ratio=[2] * 16),
        dict(field=other), dict(field=narrow), dict(field=relevelled),       # incongruent
        dict(n_levels=2),                                                     # a level >= n_levels
        dict(ratio=(2, 1)), dict(ratio=(0, 2)), dict(ratio=(-2, 2)),
        dict(index=far),
        dict(index=overlapping),                                              # two boxes of a level
        dict(field=out),                                                      # reads what it writes
    ]
    for arguments in wrong:
        assert call(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert untouched(), arguments
    with pytest.raises(ValueError, match="same number of boxes"):
        out.clumps(other, -0.5, INF, index, [2, 2])
    assert untouched()
    # ... and the call that is in order overwrites every cell and the count
    assert call() == 0
    ctx.synchronize()
    dense, n = three.reference("u", *BROAD)
    assert int(count.item()) == n
    for o, (level, lo, hi) in zip(outs, boxes):
        assert ref.same_bits(o.values.cpu().numpy(), three.cut(dense, level, lo, hi))

    # the table: `out` now holds labels
    cells = torch.full((3, n), 11, dtype=torch.int64, device=ctx.device)
    sums = torch.full((3, n), 0.25, dtype=torch.float64, device=ctx.device)
    totals = torch.full((2,), 5, dtype=torch.int64, device=ctx.device)

    def table(labels=out, field=sf, n_clumps=n, n_levels=3, with_sums=True):
        return _capi.lib().avr_scene_clump_table(
            ctx._handle, labels._handle, field._handle if field is not None else None, n_clumps,
            n_levels, C.c_void_p(cells.data_ptr()),
            C.c_void_p(sums.data_ptr()) if with_sums else None, C.c_void_p(totals.data_ptr()))

    for arguments in [dict(n_clumps=0), dict(n_levels=0), dict(n_levels=17), dict(n_levels=2),
                      dict(n_clumps=2 ** 28), dict(n_clumps=(2 ** 28 + 2) // 3),
                      dict(field=other), dict(field=narrow), dict(field=relevelled),
                      dict(field=None), dict(with_sums=False)]:
        assert table(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        ctx.synchronize()
        assert bool((cells == 11).all()) and bool((sums == 0.25).all()) and \
            bool((totals == 5).all()), arguments
    assert table() == 0                       # added to what the arrays held
    ctx.synchronize()
    masks = [m for _, m, _ in three.leaves("u")]
    want = cr.clump_table(dense, n, masks, [v for _, _, v in three.leaves("u")])
    assert np.array_equal(cells.cpu().numpy() - 11, want[0])
    assert (totals.cpu().numpy() - 5).tolist() == [0, 0]
    for scene in (sf, other, narrow, relevelled, out):
        scene.close()


# ---- the table -------------------------------------------------------------------------------------

def assert_table(got, want):
    """got: (cells, sums, totals) tensors; want: clump_reference.clump_table's tuple."""
    cells, sums, totals = got
    want_cells, want_sums, abs_sums, outside, nonfinite = want
    assert np.array_equal(cells.cpu().numpy(), want_cells)
    assert totals.cpu().numpy().tolist() == [outside, nonfinite]
    if want_sums is not None:
        # n additions in any order: (n - 1) u sum |vs|; the reference is correctly rounded: u |sum|
        bound = np.maximum(want_cells - 1, 0) * U * abs_sums + U * np.abs(want_sums)
        error = np.abs(sums.cpu().numpy() - want_sums)
        print("largest sum error / bound:", float((error / np.maximum(bound, 1e-300)).max()))
        assert (error <= bound).all()


@pytest.mark.parametrize("variable", ["u", "odd"])
def test_the_table_of_a_label_field(ctx, three, variable):
    labels, n, _ = clumps_of(ctx, three, "u", 0.4, INF)
    field = load(ctx, three, variable)
    dense = three.reference("u", 0.4, INF)[0]
    leaves = three.leaves(variable)
    masks, values = [m for _, m, _ in leaves], [v for _, _, v in leaves]
    sl = ctx.create_scene(labels.local_boxes, labels.scalar_transform)
    sf = ctx.create_scene(field.local_boxes, field.scalar_transform)
    got = sl.clump_table(n, 3, sf)
    bare = sl.clump_table(n, 3)
    ctx.synchronize()
    assert_table(got, cr.clump_table(dense, n, masks, values))
    assert bare[1] is None
    assert_table(bare, cr.clump_table(dense, n, masks))
    # too small an n: the labels above it are outside
    small = sl.clump_table(n // 2, 3, sf)
    ctx.synchronize()
    assert_table(small, cr.clump_table(dense, n // 2, masks, values))
    sl.close()
    sf.close()


def hand_made(ctx, labels, values):
    """Scenes over one box each of hand-made cells [nz, ny, nx]."""
    def scene(cells):
        t = torch.from_numpy(np.ascontiguousarray(cells)).to(ctx.device)
        nz, ny, nx = cells.shape
        return ctx.create_scene([AmrBox((0.0, 0.0, 0.0), (float(nx), float(ny), float(nz)), t, 0)],
                                ScalarTransform())
    return scene(labels), scene(values)


@pytest.mark.parametrize("shape", [(4, 4, 256), (3, 5, 131)])      # pairs, single cells
def test_waves_of_one_label_alternating_labels_and_labels_that_are_none(ctx, shape):
    rng = np.random.default_rng(46)
    k, j, i = np.indices(shape)
    values = rng.standard_normal(shape)
    values.reshape(-1)[rng.choice(values.size, 40, replace=False)] = \
        np.array([np.nan, np.inf, -np.inf, 1e300])[np.arange(40) % 4]
    mask = [np.ones(shape, dtype=bool)]
    uniform = np.full(shape, 3.0)                       # every wave holds one label
    by_row = (1 + (j + k) % 5).astype(np.float64)       # one label per row, several per workgroup
    alternating = (1 + i % 4).astype(np.float64)        # neighbouring lanes differ
    stray = alternating.copy()                          # fractional, out of range, signed zero, NaN
    flat = stray.reshape(-1)
    flat[rng.choice(flat.size, 60, replace=False)] = \
        np.array([1.5, 6.0, -1.0, -0.0, 0.0, np.nan, np.inf, 0.999, 5.0])[np.arange(60) % 9]
    for labels in (uniform, by_row, alternating, stray):
        sl, sf = hand_made(ctx, labels, values)
        got = sl.clump_table(5, 1, sf)
        bare = sl.clump_table(5, 1)
        ctx.synchronize()
        assert_table(got, cr.clump_table([labels], 5, mask, [values]))
        assert_table(bare, cr.clump_table([labels], 5, mask))
        sl.close()
        sf.close()


# ---- composition -----------------------------------------------------------------------------------

def named(ctx, case, name):
    scene = api._load_variable_scenes(ctx, case.path, [name], 0, -1, False, True, 0, 1, None)[0]
    ctx.synchronize()
    return scene


def boxes_equal(case, scene, dense):
    expected = case.scene_boxes()
    assert len(scene.local_boxes) == len(expected)
    return all(ref.same_bits(box.values.cpu().numpy(), case.cut(dense, level, lo, hi))
               for box, (level, lo, hi) in zip(scene.local_boxes, expected))


def same(a, b):
    if isinstance(a, dict):
        return all(same(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    return ref.same_bits(a, b) if a.dtype.kind == "f" else bool(np.array_equal(a, b))


def test_api_clumps_equals_the_reference(ctx, three):
    got = api.clumps(three.path, "u", *BROAD, fields=["u", "odd"])
    dense, n = three.reference("u", *BROAD)
    volumes = api.level_cell_volumes(three.sizes())
    masks = [m for _, m, _ in three.leaves("u")]
    bare = cr.clump_table(dense, n, masks)
    assert got["n"] == n and got["outside"] == 0
    assert np.array_equal(got["cells_by_level"], bare[0])
    assert np.array_equal(got["cells"], bare[0].sum(axis=0))
    volume = sum(np.float64(volumes[l]) * bare[0][l].astype(np.float64) for l in range(3))
    assert ref.same_bits(got["volume"], 0.0 + volume)
    nonfinite = 0
    for name in ("u", "odd"):
        values = [v for _, _, v in three.leaves(name)]
        cells, sums, abs_sums, _, bad = cr.clump_table(dense, n, masks, values)
        nonfinite += bad
        want = sum(np.float64(volumes[l]) * sums[l] for l in range(3))
        # per level the sum's bound, scaled by the (power of two) volume, and three additions
        bound = sum(volumes[l] * (np.maximum(cells[l] - 1, 0) * U * abs_sums[l] + U * abs(sums[l]))
                    for l in range(3)) + 3 * U * sum(volumes[l] * abs_sums[l] for l in range(3))
        assert (np.abs(got["integrals"][name] - want) <= bound).all()
    assert got["nonfinite"] == nonfinite > 0
    empty = api.clumps(three.path, "u", 50.0, 60.0, fields=["u"])
    assert empty["n"] == 0 and empty["cells_by_level"].shape == (3, 0)
    assert empty["volume"].shape == (0,) and empty["integrals"]["u"].shape == (0,)


def test_a_slice_of_a_clump_field_equals_the_stored_reference(ctx, three):
    api.add_clump_field("clump", "u", *BROAD)
    assert boxes_equal(three, named(ctx, three, "clump"), three.reference("u", *BROAD)[0])
    cut = api.slice(three.path, 40, 30, "clump", axis="y")
    assert same(cut, api.slice(three.path, 40, 30, "clump_stored", axis="y"))
    shown = set(np.unique(cut[np.isfinite(cut)]).tolist())
    assert 0.0 in shown and len(shown) >= 2          # unselected cells and at least one clump


def test_a_derived_field_over_a_clump_field_integrates_to_the_table(ctx, three):
    api.add_clump_field("clump", "u", *BROAD)
    table = api.clumps(three.path, "u", *BROAD, fields=["u"])
    k = int(np.argmax(table["cells"])) + 1
    api.add_field("in_k", f"where(clump == {k}, u, 0)")
    got = api.profile(three.path, "whole", "in_k", weight="cell_volume", bins=1)
    assert got["outside"] == 0 and got["nonfinite"] == 0
    integral = got["mean"][0] * got["weight_sum"][0]
    arrays = three.leaves("u")
    volumes = api.level_cell_volumes(three.sizes())
    dense = three.reference("u", *BROAD)[0]
    in_k = [np.abs(v[m & (d == k)]) for (_, m, v), d in zip(arrays, dense)]
    n = sum(int(m.sum()) for _, m, _ in arrays)
    weighted = sum(volumes[l] * float(in_k[l].sum()) for l in range(3))
    # both are sums of the same products in some order, each within (n - 1) u sum |vol vs| of the
    # exact value; the profile's quotient and its product back add two roundings
    bound = 2 * (n - 1) * U * weighted + 4 * U * abs(table["integrals"]["u"][k - 1])
    assert abs(integral - table["integrals"]["u"][k - 1]) <= bound
    assert weighted > 0.0 and int(table["cells"][k - 1]) > 100       # the clump is no handful of cells


def regridded(case, dense):
    return [{"domain": lev["domain"], "boxes": lev["boxes"],
             "data": [case.cut(dense, l, *box)[None] for box in lev["boxes"]]}
            for l, lev in enumerate(case.levels)]


def test_a_clump_field_of_a_gradient_field(ctx, three):
    api.add_gradient_field("du_dx", "u", "x")
    api.add_clump_field("steep", "du_dx", 2.0)
    gradient = ref.gradient_levels(three.levels, three.ratio, three.sizes(), 0, 0)[0]
    want, n = cr.clump_levels(regridded(three, gradient), three.ratio, 0, 2.0, INF,
                              three.scene_boxes())
    assert n > 3 and boxes_equal(three, named(ctx, three, "steep"), want)


def test_products_of_stored_variables_are_unchanged_around_clumps(ctx, three, tmp_path):
    def products():
        out = str(tmp_path / "frame.ppm")
        assert api.run(three.path, api.RenderOptions(width=96, height=64, output_filename=out),
                       "u", ctx) == 0
        with open(out, "rb") as fh:
            frame = fh.read()
        return (api.slice(three.path, 40, 30, "u", axis="y"),
                api.project_axis(three.path, "z", "u", None, 53, 41), frame)

    before = products()
    api.add_clump_field("clump", "u", *BROAD)
    during = products()
    assert api.clumps(three.path, "u", *BROAD)["n"] > 1
    assert np.isfinite(api.slice(three.path, 40, 30, "clump", axis="y")).sum() > 500
    after = products()
    for a, b, c in zip(before, during, after):
        if isinstance(a, bytes):
            assert a == b == c
        else:
            assert same(a, b) and same(a, c)
