"""Isosurfaces on the GPU: the kernels of avr_isosurface.hip through avr_scene_isosurface,
api.isosurface_scene and api.isosurface, against the numpy reference on the plotfile's own level
arrays (isosurface_reference).  Vertices, levels and samples are equal by bits, the counts are
equal.  Cell sizes are powers of two, and every coarse cell that a finer grid covers holds 1e30: a
read of a parent grid past a leaf box's view would show as a wrong vertex."""
import ctypes as C
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, plotfile, surfaces

import gradient_reference as ref
import isosurface_reference as iso

pytestmark = pytest.mark.gpu
VARIABLES = list(ref.VARIABLES)


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
    def reference(self, variable, value, min_level=0, max_level=-1, sample=None):
        return iso.isosurface(self.levels, self.ratio, VARIABLES.index(variable), value,
                              self.scene_boxes(min_level, max_level), self.sizes(), self.lo,
                              min_level, max_level,
                              None if sample is None else VARIABLES.index(sample))


def _write(path, domains, boxes, lo, hi, ratio, seed):
    levels = ref.make_levels(domains, boxes, ratio, seed)
    case = Case(str(path), levels, lo, hi, list(ratio))
    for size in case.sizes():
        assert all(np.frexp(s)[0] == 0.5 for s in size)             # powers of two
    plotfile.write_plotfile(str(path), VARIABLES, levels, lo, hi, ratio)
    return case


THREE_DOMAINS = [((0, 0, 0), (11, 5, 7)), ((0, 0, 0), (23, 11, 15)), ((0, 0, 0), (47, 23, 31))]
# two fine boxes that touch at i = 11 | 12; the finest grid lies inside the first
THREE_BOXES = [[((0, 0, 0), (6, 5, 7)), ((7, 0, 0), (11, 5, 7))],
               [((4, 2, 2), (11, 7, 9)), ((12, 2, 2), (17, 9, 9))],
               [((12, 6, 6), (21, 13, 15))]]


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("iso") / "three", THREE_DOMAINS, THREE_BOXES,
                  (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 2], 61)


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    grids = [((0, 0, 0), (130, 4, 2)), ((131, 0, 0), (386, 3, 3)), ((387, 0, 0), (387, 3, 3)),
             ((388, 0, 0), (390, 3, 3)), ((395, 7, 7), (395, 7, 7))]
    return _write(tmp_path_factory.mktemp("iso") / "shapes", [((0, 0, 0), (399, 7, 7))],
                  [grids], (0.0, 0.0, 0.0), (100.0, 2.0, 2.0), [], 62)


@pytest.fixture(scope="module")
def ratio_four(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("iso") / "four",
                  [((0, 0, 0), (5, 3, 3)), ((0, 0, 0), (23, 15, 15))],
                  [[((0, 0, 0), (5, 3, 3))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (3.0, 2.0, 2.0), [4], 63)


@pytest.fixture(scope="module")
def skipped_level(tmp_path_factory):
    """The finest grid covers the low-x half of the middle one: a level-0 leaf lies face to face
    with level-2 cells."""
    return _write(tmp_path_factory.mktemp("iso") / "skipped",
                  [((0, 0, 0), (7, 3, 3)), ((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))],
                  [[((0, 0, 0), (7, 3, 3))], [((4, 2, 2), (11, 5, 5))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [2, 2], 64)


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    grids = [((4 * a, 4 * b, 4 * c), (4 * a + 3, 4 * b + 3, 4 * c + 3))
             for c in range(5) for b in range(4) for a in range(4)]
    return _write(tmp_path_factory.mktemp("iso") / "many", [((0, 0, 0), (15, 15, 19))],
                  [grids], (0.0, 0.0, 0.0), (2.0, 2.0, 2.5), [], 65)


def load(ctx, case, name, min_level=0, max_level=-1):
    return plotfile.load_plotfile_geometry(ctx, case.path, name, min_level, max_level, False, True)


def same_surface(got, want):
    vertices, levels, samples, skipped = got
    print("triangles:", vertices.shape[0], "reference:", want["vertices"].shape[0],
          "skipped:", skipped, "reference:", want["skipped"])
    assert vertices.shape == want["vertices"].shape and skipped == want["skipped"]
    assert ref.same_bits(vertices, want["vertices"])
    assert levels.dtype == np.uint8 and np.array_equal(levels, want["level"])
    if want["samples"] is None:
        assert samples is None
    else:
        assert ref.same_bits(samples, want["samples"])


def check(ctx, case, variable, value, min_level=0, max_level=-1, sample=None):
    scene = load(ctx, case, variable, min_level, max_level)
    other = load(ctx, case, sample, min_level, max_level) if sample is not None else None
    finest = max(b.level for b in scene.all_boxes)
    got = api.isosurface_scene(ctx, scene, value, case.sizes()[:finest + 1], case.lo,
                               case.ratio[:finest], other)
    want = case.reference(variable, value, min_level, max_level, sample)
    same_surface(got, want)
    return got, scene


def pair_path(scene):
    even = lambda b: (b.values.data_ptr() % 16 == 0 and b.values.stride(1) % 2 == 0 and
                      b.values.stride(0) % 2 == 0)
    return [even(b) for b in scene.local_boxes]


# ---- hierarchy -----------------------------------------------------------------------------------

def test_three_levels_with_fine_boxes_that_touch(ctx, three):
    (vertices, levels, _, _), scene = check(ctx, three, "u", 0.1)
    paths = pair_path(scene)
    assert any(paths) and not all(paths)          # leaf boxes are odd-strided views of their grids
    assert set(levels.tolist()) == {0, 1, 2} and vertices.shape[0] > 5000
    # cubes whose corners come from a coarser level, by the reference's own cubes
    cubes = three.reference("u", 0.1)["cubes"]
    assert any(l == 2 and i == 11 for _, l, (i, _, _) in cubes)
    check(ctx, three, "u", 1.5)                   # few cubes cut


def test_ratio_four(ctx, ratio_four):
    check(ctx, ratio_four, "u", 0.0)
    check(ctx, ratio_four, "u", 0.7)


def test_a_coarse_leaf_face_to_face_with_cells_two_levels_finer(ctx, skipped_level):
    check(ctx, skipped_level, "u", 0.2)
    cubes = skipped_level.reference("u", 0.2)["cubes"]
    assert any(l == 2 and i == 7 for _, l, (i, _, _) in cubes)       # their low-x rim: level 0


@pytest.mark.parametrize("levels", [(1, -1), (0, 0)])
def test_level_ranges_leave_holes_and_whole_coarse_grids(ctx, three, levels):
    check(ctx, three, "u", 0.1, *levels)


def test_eighty_boxes(ctx, many):
    (vertices, _, _, _), scene = check(ctx, many, "u", 0.3)
    assert len(scene.local_boxes) == 80 and vertices.shape[0] > 5000


def test_rows_of_131_and_256_cells_a_thin_box_and_a_lone_cell(ctx, shapes):
    _, scene = check(ctx, shapes, "u", -0.2)
    assert pair_path(scene) == [False, True, False, False, False]
    assert [b.cell_dimensions for b in scene.local_boxes] == [(131, 5, 3), (256, 4, 4), (1, 4, 4),
                                                              (3, 4, 4), (1, 1, 1)]
    check(ctx, shapes, "u", 1.0)


# ---- values --------------------------------------------------------------------------------------

def test_cubes_with_nan_and_infinite_corners_are_skipped_and_counted(ctx, three):
    (_, _, _, skipped), _ = check(ctx, three, "odd", 0.1)
    assert skipped > 50


def test_a_value_that_cells_hold_gives_degenerate_triangles(ctx, three):
    arrays = ref.leaf_arrays(three.levels, three.ratio, VARIABLES.index("whole"))[0]
    held = np.sort(np.concatenate([v[m] for _, m, v in arrays]))
    # the median and the upper quartile: the cell that holds `value` is inside, and a triangle
    # degenerates only where at most one other vertex of its tetrahedron is inside as well (with
    # three inside vertices the triangle merely has one corner at that cell), which needs enough
    # cells below `value` around it
    for value in (float(held[len(held) // 2]), float(held[3 * len(held) // 4])):
        (vertices, _, _, _), _ = check(ctx, three, "whole", value)
        areas = surfaces.triangle_areas(vertices)
        # a tetrahedron whose one inside vertex holds `value` gives a triangle of three equal points
        assert (areas == 0.0).any() and (areas > 0.0).any()
        assert (vertices[:, 0] == vertices[:, 1]).all(axis=1).any()


def test_a_value_above_the_maximum_gives_no_triangle(ctx, shapes):
    (vertices, levels, samples, skipped), _ = check(ctx, shapes, "u", 100.0, sample="whole")
    assert vertices.shape == (0, 3, 3) and levels.shape == (0,) and samples.shape == (0, 3)
    assert skipped == 0


def test_a_sample_scene_is_interpolated_at_every_vertex(ctx, three, ratio_four):
    (_, _, samples, _), _ = check(ctx, three, "u", 0.1, sample="whole")
    assert samples.shape[1] == 3 and np.isfinite(samples).all()
    check(ctx, three, "odd", -0.3, sample="odd")     # its own values: `value` at every vertex
    check(ctx, ratio_four, "u", 0.0, sample="whole")


def test_a_repeat_gives_equal_bits(ctx, three):
    scene = load(ctx, three, "odd")
    other = load(ctx, three, "u")
    runs = [api.isosurface_scene(ctx, scene, -0.3, three.sizes(), three.lo, three.ratio, other)
            for _ in range(2)]
    assert runs[0][3] == runs[1][3] and np.array_equal(runs[0][1], runs[1][1])
    assert ref.same_bits(runs[0][0], runs[1][0]) and ref.same_bits(runs[0][2], runs[1][2])


# ---- the C ABI -------------------------------------------------------------------------------------

def test_wrong_arguments_are_refused_and_a_small_capacity_leaves_the_outputs_untouched(ctx, three):
    f = load(ctx, three, "u")
    w = load(ctx, three, "whole")
    coarse = load(ctx, three, "u", 0, 0)
    sf = ctx.create_scene(f.local_boxes, f.scalar_transform)
    sw = ctx.create_scene(w.local_boxes, w.scalar_transform)
    other = ctx.create_scene(coarse.local_boxes, coarse.scalar_transform)
    narrow = ctx.create_scene([dataclasses.replace(f.local_boxes[0],
                                                   values=f.local_boxes[0].values[:, :, :-1])]
                              + f.local_boxes[1:], f.scalar_transform)
    relevelled = ctx.create_scene(f.local_boxes[:-1] + [dataclasses.replace(f.local_boxes[-1],
                                                                             level=0)],
                                  f.scalar_transform)
    want = three.reference("u", 0.1, 0, -1, "whole")
    total = want["vertices"].shape[0]
    vertices = torch.full((total, 3, 3), 0.5, dtype=torch.float64, device=ctx.device)
    levels = torch.full((total,), 7, dtype=torch.uint8, device=ctx.device)
    samples = torch.full((total, 3), 0.25, dtype=torch.float64, device=ctx.device)
    counts = torch.full((2,), -7, dtype=torch.int64, device=ctx.device)
    boxes = three.scene_boxes()
    index = np.array([lo for _, lo, _ in boxes], dtype=np.int32)

    def arrays_untouched():
        ctx.synchronize()
        return bool((vertices == 0.5).all()) and bool((levels == 7).all()) and \
            bool((samples == 0.25).all())

    def call(field=sf, sample=sw, value=0.1, index=index, ratio=(2, 2), sizes=None, prob_lo=None,
             n_levels=3, capacity=total, vertices=vertices, levels=levels, samples=samples,
             counts=counts):
        index = np.ascontiguousarray(index, np.int32)
        ratio = np.ascontiguousarray(ratio, np.int32)
        sizes = np.ascontiguousarray(three.sizes() if sizes is None else sizes, np.float64)
        prob_lo = np.ascontiguousarray(three.lo if prob_lo is None else prob_lo, np.float64)
        pointer = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        return _capi.lib().avr_scene_isosurface(
            ctx._handle, field._handle, sample._handle if sample is not None else None, value,
            index.ctypes.data_as(C.POINTER(C.c_int32)), ratio.ctypes.data_as(C.POINTER(C.c_int32)),
            sizes.ctypes.data_as(C.POINTER(C.c_double)),
            prob_lo.ctypes.data_as(C.POINTER(C.c_double)), n_levels, capacity, pointer(vertices),
            pointer(levels), pointer(samples), pointer(counts))

    overlapping = index.copy()
    same_level = [b for b, (level, _, _) in enumerate(boxes) if level == 1]
    overlapping[same_level[1]] = index[same_level[0]]
    far = index.copy()
    far[0, 0] = 2 ** 30
    bad_sizes = np.array(three.sizes())
    bad_sizes[1, 2] = 0.0
    inside = f.local_boxes[1].values          # an output array that is an input box's cells
    wrong = [
        dict(value=math.nan), dict(value=math.inf), dict(value=-math.inf),
        dict(n_levels=0), dict(n_levels=17, ratio=[2] * 16, sizes=np.ones((17, 3))),
        dict(sizes=bad_sizes), dict(sizes=-np.array(three.sizes())),
        dict(prob_lo=(0.0, math.nan, 0.0)), dict(prob_lo=(math.inf, 0.0, 0.0)),
        dict(capacity=2 ** 36),
        dict(vertices=None), dict(levels=None), dict(samples=None), dict(sample=None),
        dict(counts=None),
        dict(sample=other), dict(sample=narrow), dict(sample=relevelled),     # incongruent
        dict(field=other), dict(n_levels=2),                                  # a level >= n_levels
        dict(ratio=(2, 1)), dict(ratio=(0, 2)), dict(ratio=(-2, 2)),
        dict(index=far),
        dict(index=overlapping),                                              # two boxes of a level
        dict(capacity=1, samples=inside), dict(capacity=0, counts=inside),    # writes what it reads
    ]
    for arguments in wrong:
        assert call(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert arrays_untouched() and counts.tolist() == [-7, -7], arguments
    # a capacity one below T: the counts are written, the arrays are not
    assert call(capacity=total - 1) == 0
    assert arrays_untouched() and counts.tolist() == [total, want["skipped"]]
    counts.fill_(-7)
    assert call(capacity=0, vertices=None, levels=None, samples=None) == 0      # the count-only call
    assert arrays_untouched() and counts.tolist() == [total, want["skipped"]]
    # ... and the call that is in order writes everything
    assert call() == 0
    ctx.synchronize()
    same_surface((vertices.cpu().numpy(), levels.cpu().numpy(), samples.cpu().numpy(),
                  int(counts[1].item())), want)
    for scene in (sf, sw, other, narrow, relevelled):
        scene.close()


# ---- composition -----------------------------------------------------------------------------------

def regridded(case, dense):
    dlo = [lev["domain"][0] for lev in case.levels]
    cut = lambda l, lo, hi: dense[l][lo[2] - dlo[l][2]:hi[2] - dlo[l][2] + 1,
                                     lo[1] - dlo[l][1]:hi[1] - dlo[l][1] + 1,
                                     lo[0] - dlo[l][0]:hi[0] - dlo[l][0] + 1]
    return [{"domain": lev["domain"], "boxes": lev["boxes"],
             "data": [cut(l, *box)[None] for box in lev["boxes"]]}
            for l, lev in enumerate(case.levels)]


def test_api_isosurface_of_a_stored_a_derived_and_a_gradient_field(ctx, three, tmp_path):
    out = str(tmp_path / "surface.ply")
    got = api.isosurface(three.path, "u", 0.1, fields=["whole", "u"], output=out)
    want = three.reference("u", 0.1, 0, -1, "whole")
    n = want["vertices"].shape[0]
    assert got["n"] == n and got["skipped"] == 0 and np.array_equal(got["level"], want["level"])
    assert ref.same_bits(got["vertices"], want["vertices"])
    assert ref.same_bits(got["samples"]["whole"], want["samples"])
    assert ref.same_bits(got["samples"]["u"], three.reference("u", 0.1, 0, -1, "u")["samples"])
    assert ref.same_bits(got["area"], surfaces.triangle_areas(want["vertices"]))
    assert got["total_area"] == math.fsum(got["area"].tolist()) > 0.0
    back, samples = surfaces.load_ply(out)
    assert ref.same_bits(back, want["vertices"]) and list(samples) == ["whole", "u"]
    assert api.isosurface(three.path, "u", 50.0)["n"] == 0

    api.add_field("twice", "u + u")
    doubled = [{"domain": lev["domain"], "boxes": lev["boxes"],
                "data": [d[0:1] + d[0:1] for d in lev["data"]]} for lev in three.levels]
    want = iso.isosurface(doubled, three.ratio, 0, 0.2, three.scene_boxes(), three.sizes(), three.lo)
    got = api.isosurface(three.path, "twice", 0.2)
    assert got["n"] == want["vertices"].shape[0] > 1000
    assert ref.same_bits(got["vertices"], want["vertices"])

    api.add_gradient_field("du_dx", "u", "x")
    gradient = ref.gradient_levels(three.levels, three.ratio, three.sizes(), 0, 0)[0]
    want = iso.isosurface(regridded(three, gradient), three.ratio, 0, 2.0, three.scene_boxes(),
                          three.sizes(), three.lo)
    got = api.isosurface(three.path, "du_dx", 2.0, min_level=0)
    assert got["n"] == want["vertices"].shape[0] > 1000
    assert ref.same_bits(got["vertices"], want["vertices"])
    assert np.array_equal(got["level"], want["level"])


def test_a_slice_of_a_stored_variable_is_unchanged_around_an_isosurface(ctx, three):
    before = api.slice(three.path, 40, 30, "u", axis="y")
    assert api.isosurface(three.path, "u", 0.1, fields=["odd"])["n"] > 1000
    after = api.slice(three.path, 40, 30, "u", axis="y")
    assert ref.same_bits(before, after)
