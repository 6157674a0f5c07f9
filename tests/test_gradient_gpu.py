"""Gradient fields on the GPU: gradient_halo_kernel and gradient_kernel through avr_scene_gradient,
api.gradient_scene and the registry, against the numpy reference on the plotfile's own level
arrays (gradient_reference).  Equality is by bits, NaN equal to NaN, with no tolerance anywhere:
every operation is correctly rounded and the order of the additions is fixed.  Cell sizes are
powers of two, and every coarse cell that a finer grid covers holds 1e30: a read of a parent grid
past a leaf box's view would show in the result."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, plotfile
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform

import gradient_reference as ref

pytestmark = pytest.mark.gpu
VARIABLES = list(ref.VARIABLES)


@pytest.fixture(autouse=True)
def _empty_registries():
    def clear():
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
    def reference(self, variable, axis, min_level=0, max_level=-1):
        return ref.gradient_levels(self.levels, self.ratio, self.sizes(), axis,
                                   VARIABLES.index(variable), min_level, max_level)[0]

    def cut(self, dense, level, lo, hi):
        dlo = self.levels[level]["domain"][0]
        return dense[level][lo[2] - dlo[2]:hi[2] - dlo[2] + 1, lo[1] - dlo[1]:hi[1] - dlo[1] + 1,
                            lo[0] - dlo[0]:hi[0] - dlo[0] + 1]


def _write(path, domains, boxes, lo, hi, ratio, seed, extra=None):
    levels = ref.make_levels(domains, boxes, ratio, seed)
    case = Case(str(path), levels, lo, hi, list(ratio))
    for size in case.sizes():
        assert all(np.frexp(s)[0] == 0.5 for s in size)             # powers of two
    names, written = VARIABLES, levels
    if extra is not None:
        more = extra(case)
        names = VARIABLES + list(more)
        written = [{"domain": lev["domain"], "boxes": lev["boxes"],
                    "data": [np.concatenate([data] + [case.cut(dense, l, *box)[None]
                                                      for dense in more.values()])
                             for box, data in zip(lev["boxes"], lev["data"])]}
                   for l, lev in enumerate(levels)]
    plotfile.write_plotfile(str(path), names, written, lo, hi, ratio)
    return case


THREE_DOMAINS = [((0, 0, 0), (11, 5, 7)), ((0, 0, 0), (23, 11, 15)), ((0, 0, 0), (47, 23, 31))]
# two fine boxes that touch at i = 11 | 12; the finest grid lies inside the first
THREE_BOXES = [[((0, 0, 0), (6, 5, 7)), ((7, 0, 0), (11, 5, 7))],
               [((4, 2, 2), (11, 7, 9)), ((12, 2, 2), (17, 9, 9))],
               [((12, 6, 6), (21, 13, 15))]]


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    """Three levels at ratio 2, non-cubic, coarse cells of 1/8 x 1/4 x 1/8; stored next to the
    fields: the reference's du/dx, so that products of the gradient field have a stored twin."""
    twins = lambda case: {"du_dx_stored": case.reference("u", 0)}
    return _write(tmp_path_factory.mktemp("gradient") / "three", THREE_DOMAINS, THREE_BOXES,
                  (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 2], 31, twins)


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    """One level: 131 x 5 x 3 (odd strides: single cells) next to 256 x 4 x 4 (pairs) along x, a
    box one cell wide along x between two others, and an isolated cell."""
    grids = [((0, 0, 0), (130, 4, 2)), ((131, 0, 0), (386, 3, 3)), ((387, 0, 0), (387, 3, 3)),
             ((388, 0, 0), (390, 3, 3)), ((395, 7, 7), (395, 7, 7))]
    return _write(tmp_path_factory.mktemp("gradient") / "shapes", [((0, 0, 0), (399, 7, 7))],
                  [grids], (0.0, 0.0, 0.0), (100.0, 2.0, 2.0), [], 32)


@pytest.fixture(scope="module")
def ratio_four(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("gradient") / "four",
                  [((0, 0, 0), (5, 3, 3)), ((0, 0, 0), (23, 15, 15))],
                  [[((0, 0, 0), (5, 3, 3))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (3.0, 2.0, 2.0), [4], 33)


@pytest.fixture(scope="module")
def skipped_level(tmp_path_factory):
    """The finest grid covers the low-x half of the middle one: a level-0 leaf lies face to face
    with level-2 cells, its ghost's children are no leaves (absent), while theirs is that leaf."""
    return _write(tmp_path_factory.mktemp("gradient") / "skipped",
                  [((0, 0, 0), (7, 3, 3)), ((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))],
                  [[((0, 0, 0), (7, 3, 3))], [((4, 2, 2), (11, 5, 5))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [2, 2], 34)


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    grids = [((4 * a, 4 * b, 4 * c), (4 * a + 3, 4 * b + 3, 4 * c + 3))
             for c in range(5) for b in range(4) for a in range(4)]
    return _write(tmp_path_factory.mktemp("gradient") / "many", [((0, 0, 0), (15, 15, 19))],
                  [grids], (0.0, 0.0, 0.0), (2.0, 2.0, 2.5), [], 35)


def load(ctx, case, name, min_level=0, max_level=-1):
    return plotfile.load_plotfile_geometry(ctx, case.path, name, min_level, max_level, False, True)


def gradient_of(ctx, case, variable, axis, min_level=0, max_level=-1):
    scene = load(ctx, case, variable, min_level, max_level)
    finest = max(b.level for b in scene.all_boxes)
    out = api.gradient_scene(ctx, scene, axis, case.sizes()[:finest + 1], case.lo, case.ratio)
    ctx.synchronize()
    return out, scene


def pair_path(scene, out):
    """Per box whether the kernel takes f64 pairs: input and output 16-byte aligned, even strides."""
    even = lambda b: (b.values.data_ptr() % 16 == 0 and b.values.stride(1) % 2 == 0 and
                      b.values.stride(0) % 2 == 0)
    return [even(a) and even(b) for a, b in zip(scene.local_boxes, out.local_boxes)]


def check(ctx, case, variable, axis, min_level=0, max_level=-1):
    out, scene = gradient_of(ctx, case, variable, axis, min_level, max_level)
    dense = case.reference(variable, axis, min_level, max_level)
    expected = case.scene_boxes(min_level, max_level)
    assert len(out.local_boxes) == len(out.all_boxes) == len(expected) > 0
    assert out.world_scale == scene.world_scale
    for box, (level, lo, hi) in zip(out.local_boxes, expected):
        assert box.level == level
        assert box.cell_dimensions == tuple(hi[a] - lo[a] + 1 for a in range(3))
        assert box.values.is_contiguous() and box.values.data_ptr() % 16 == 0
        assert ref.same_bits(box.values.cpu().numpy(), case.cut(dense, level, lo, hi)), \
            (variable, axis, level, lo, hi)
    return out, scene


# ---- the kernels against the reference -----------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_three_levels_equal_the_reference_on_every_axis(ctx, three, axis):
    out, scene = check(ctx, three, "u", axis)
    assert {b.level for b in out.local_boxes} == {0, 1, 2}
    paths = pair_path(scene, out)
    assert any(paths) and not all(paths)          # leaf boxes are odd-strided views of their grids
    check(ctx, three, "odd", axis)                # about 2 % NaN / +Inf / -Inf
    check(ctx, three, "whole", axis)              # integers
    again = gradient_of(ctx, three, "odd", axis)[0]
    first = gradient_of(ctx, three, "odd", axis)[0]
    for a, b in zip(again.local_boxes, first.local_boxes):
        assert ref.same_bits(a.values.cpu().numpy(), b.values.cpu().numpy())


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_rows_of_131_and_256_cells_a_thin_box_and_a_lone_cell(ctx, shapes, axis):
    out, scene = check(ctx, shapes, "u", axis)
    assert pair_path(scene, out) == [False, True, False, False, False]
    assert [b.cell_dimensions for b in out.local_boxes] == [(131, 5, 3), (256, 4, 4), (1, 4, 4),
                                                            (3, 4, 4), (1, 1, 1)]
    assert out.local_boxes[4].values.cpu().numpy().tolist() == [[[0.0]]]     # no neighbour at all
    if axis == 0:
        # the box one cell wide has both neighbours: the central difference of the boxes beside it
        u = ref.leaf_arrays(shapes.levels, [], 0)[0][0][2]
        want = (u[0:4, 0:4, 388] - u[0:4, 0:4, 386]) / (2.0 * shapes.sizes()[0][0])
        assert ref.same_bits(out.local_boxes[2].values.cpu().numpy()[:, :, 0], want)
    check(ctx, shapes, "odd", axis)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_ratio_four_restricts_sixty_four_children(ctx, ratio_four, axis):
    check(ctx, ratio_four, "u", axis)
    check(ctx, ratio_four, "odd", axis)


@pytest.mark.parametrize("levels", [(1, -1), (0, 0), (1, 1), (0, 1)])
def test_level_ranges_leave_holes_and_whole_coarse_grids(ctx, three, levels):
    for axis in range(3):
        check(ctx, three, "u", axis, *levels)


def test_a_coarse_leaf_next_to_cells_two_levels_finer_has_no_ghost_there(ctx, skipped_level):
    case = skipped_level
    arrays, _ = ref.leaf_arrays(case.levels, case.ratio, 0)
    assert arrays[0][1][1, 1, 1] and not arrays[0][1][1, 1, 2] and not arrays[1][1][2, 2, 4]
    dense = case.reference("u", 0)
    u0 = arrays[0][2]
    one_sided = (u0[1, 1, 1] - u0[1, 1, 0]) / case.sizes()[0][0]
    assert ref.same_bits(dense[0][1, 1, 1], one_sided)
    for axis in range(3):
        check(ctx, case, "u", axis)
        check(ctx, case, "odd", axis)


def test_eighty_boxes(ctx, many):
    for axis in range(3):
        out, _ = check(ctx, many, "u", axis)
        assert len(out.local_boxes) == 80


# ---- the C ABI's checks ----------------------------------------------------------------------------

def test_wrong_arguments_are_refused_and_the_output_untouched(ctx, three):
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
    boxes = three.scene_boxes()
    index = np.array([lo for _, lo, _ in boxes], dtype=np.int32)
    sizes = np.array([s[0] for s in three.sizes()])

    def untouched():
        ctx.synchronize()
        return all(bool((b.values == sentinel).all()) for b in outs)

    def call(field=sf, target=out, axis=0, index=index, ratio=(2, 2), sizes=sizes, n_levels=None):
        index = np.ascontiguousarray(index, np.int32)
        ratio = np.ascontiguousarray(ratio, np.int32)
        sizes = np.ascontiguousarray(sizes, np.float64)
        return _capi.lib().avr_scene_gradient(
            ctx._handle, field._handle, target._handle, axis,
            index.ctypes.data_as(C.POINTER(C.c_int32)), ratio.ctypes.data_as(C.POINTER(C.c_int32)),
            sizes.ctypes.data_as(C.POINTER(C.c_double)),
            sizes.size if n_levels is None else n_levels)

    overlapping = index.copy()
    same_level = [b for b, (level, _, _) in enumerate(boxes) if level == 1]
    overlapping[same_level[1]] = index[same_level[0]]
    wrong = [
        dict(axis=3), dict(axis=-1),
        dict(field=other), dict(field=narrow), dict(field=relevelled),       # incongruent
        dict(n_levels=2), dict(n_levels=0),                                   # a level >= n_levels
        dict(n_levels=17, sizes=np.ones(17), ratio=[2] * 16),
        dict(ratio=(2, 1)), dict(ratio=(0, 2)), dict(ratio=(-2, 2)),
        dict(sizes=[0.125, np.inf, 0.03125]), dict(sizes=[0.125, np.nan, 0.03125]),
        dict(sizes=[0.125, 0.0, 0.03125]), dict(sizes=[-0.125, 0.0625, 0.03125]),
        dict(field=out),                                                      # reads what it writes
        dict(index=overlapping),                                              # two boxes of a level
    ]
    for arguments in wrong:
        assert call(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert untouched(), arguments
    with pytest.raises(ValueError, match="same number of boxes"):
        out.gradient(other, 0, index, [2, 2], sizes)
    assert untouched()
    # ... and the call that is in order overwrites every cell
    assert call() == 0
    ctx.synchronize()
    dense = three.reference("u", 0)
    for o, (level, lo, hi) in zip(outs, boxes):
        assert ref.same_bits(o.values.cpu().numpy(), three.cut(dense, level, lo, hi))


# ---- through the registry --------------------------------------------------------------------------

def named(ctx, case, name):
    scene = api._load_variable_scenes(ctx, case.path, [name], 0, -1, False, True, 0, 1, None)[0]
    ctx.synchronize()
    return scene


def boxes_equal(case, scene, dense):
    expected = case.scene_boxes()
    assert len(scene.local_boxes) == len(expected)
    return all(ref.same_bits(box.values.cpu().numpy(), case.cut(dense, level, lo, hi))
               for box, (level, lo, hi) in zip(scene.local_boxes, expected))


def regridded(case, dense):
    """levels whose only field is `dense` (per level, over the domain), cut to the grids."""
    return [{"domain": lev["domain"], "boxes": lev["boxes"],
             "data": [case.cut(dense, l, *box)[None] for box in lev["boxes"]]}
            for l, lev in enumerate(case.levels)]


def test_vorticity_through_both_registries_equals_the_reference(ctx, three):
    api.add_gradient_field("dvy_dx", "whole", "x")
    api.add_gradient_field("dux_dy", "u", "y")
    api.add_field("vort_z", "field('dvy_dx') - field('dux_dy')")
    with np.errstate(all="ignore"):
        want = [a - b for a, b in zip(three.reference("whole", 0), three.reference("u", 1))]
    assert boxes_equal(three, named(ctx, three, "vort_z"), want)


def test_a_gradient_of_a_derived_field_and_a_second_derivative(ctx, three):
    api.add_field("sq", "u * u + whole")
    api.add_gradient_field("dsq_dz", "sq", 2)
    _, masks_u = ref.gradient_levels(three.levels, three.ratio, three.sizes(), 2, 0)
    _, masks_w = ref.gradient_levels(three.levels, three.ratio, three.sizes(), 2, 2)
    sq = [u[2] * u[2] + w[2] for u, w in zip(masks_u, masks_w)]
    want = ref.gradient_levels(regridded(three, sq), three.ratio, three.sizes(), 2, 0)[0]
    assert boxes_equal(three, named(ctx, three, "dsq_dz"), want)

    api.add_gradient_field("du_dx", "u", 0)
    api.add_gradient_field("d2u_dx2", "du_dx", "x")
    first = three.reference("u", 0)
    want = ref.gradient_levels(regridded(three, first), three.ratio, three.sizes(), 0, 0)[0]
    assert boxes_equal(three, named(ctx, three, "d2u_dx2"), want)


def same(a, b):
    if isinstance(a, dict):
        return all(same(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is b
    a, b = np.asarray(a), np.asarray(b)
    return ref.same_bits(a, b) if a.dtype.kind == "f" else bool(np.array_equal(a, b))


def test_a_slice_and_a_profile_of_a_gradient_field_equal_the_stored_reference(ctx, three):
    """du_dx_stored holds the reference's arrays (written by the fixture): the products of the
    gradient field must equal those of the stored numpy result bit for bit."""
    api.add_gradient_field("du_dx", "u", "x")
    cut = api.slice(three.path, 40, 30, "du_dx", axis="y")
    assert same(cut, api.slice(three.path, 40, 30, "du_dx_stored", axis="y"))
    assert np.isfinite(cut).sum() > 500 and len(np.unique(cut[np.isfinite(cut)])) > 50
    got = api.profile(three.path, "du_dx", "whole", weight="cells", bins=16)
    want = api.profile(three.path, "du_dx_stored", "whole", weight="cells", bins=16)
    assert same(got, want) and got["cells"].sum() > 1000


def test_products_of_stored_variables_are_unchanged_around_a_gradient(ctx, three, tmp_path):
    def products():
        out = str(tmp_path / "frame.ppm")
        assert api.run(three.path, api.RenderOptions(width=96, height=64, output_filename=out),
                       "u", ctx) == 0
        with open(out, "rb") as fh:
            frame = fh.read()
        return (api.slice(three.path, 40, 30, "u", axis="y"),
                api.project_axis(three.path, "z", "u", None, 53, 41), frame)

    before = products()
    api.add_gradient_field("du_dz", "u", "z")
    during = products()
    assert np.isfinite(api.slice(three.path, 40, 30, "du_dz", axis="y")).sum() > 500
    after = products()
    for a, b, c in zip(before, during, after):
        if isinstance(a, bytes):
            assert a == b == c
        else:
            assert same(a, b) and same(a, c)
