"""Covering grids on the GPU: the kernel of avr_covering_grid.hip through avr_scene_covering_grid,
api.covering_grid_scene and api.covering_grid, against the numpy reference on the plotfile's own
level arrays (covering_grid_reference).  Values and coverages are equal by bits, the cell levels
are equal.  Every coarse cell that a finer grid covers holds 1e30: a read of a parent grid past a
leaf box's view would show as a wrong value."""
import ctypes as C
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, grids, plotfile, runtime

import covering_grid_reference as cg
import derive_reference
import gradient_reference as ref

pytestmark = pytest.mark.gpu
VARIABLES = list(ref.VARIABLES)
NAN_PAYLOAD = float(np.array([0x7ff8000000001234], dtype=np.uint64).view(np.float64)[0])


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

    def whole(self, level):
        return cg.whole_domain(self.levels, self.ratio, level)

    @functools.lru_cache(maxsize=None)
    def reference(self, variable, level, lo, dims, min_level=0, max_level=-1, fill=math.nan):
        return cg.covering_grid(self.levels, self.ratio, VARIABLES.index(variable), level, lo,
                                dims, fill, min_level, max_level)


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
    return _write(tmp_path_factory.mktemp("grid") / "three", THREE_DOMAINS, THREE_BOXES,
                  (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 2], 71)


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    grids_ = [((0, 0, 0), (130, 4, 2)), ((131, 0, 0), (386, 3, 3)), ((387, 0, 0), (387, 3, 3)),
              ((388, 0, 0), (390, 3, 3)), ((395, 7, 7), (395, 7, 7))]
    return _write(tmp_path_factory.mktemp("grid") / "shapes", [((0, 0, 0), (399, 7, 7))],
                  [grids_], (0.0, 0.0, 0.0), (100.0, 2.0, 2.0), [], 72)


@pytest.fixture(scope="module")
def ratio_four(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("grid") / "four",
                  [((0, 0, 0), (5, 3, 3)), ((0, 0, 0), (23, 15, 15))],
                  [[((0, 0, 0), (5, 3, 3))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (3.0, 2.0, 2.0), [4], 73)


def load(ctx, case, name, min_level=0, max_level=-1):
    return plotfile.load_plotfile_geometry(ctx, case.path, name, min_level, max_level, False, True)


def same_grid(got, want):
    values, coverage, cell_level = got
    print("cells:", values.size, "classes:", cg.class_counts(want), "got:",
          cg.class_counts({"level": cell_level}))
    assert values.shape == want["values"].shape and values.dtype == np.float64
    assert cell_level.dtype == np.int8 and np.array_equal(cell_level, want["level"])
    assert ref.same_bits(coverage, want["coverage"])
    assert ref.same_bits(values, want["values"])


def grid_of(ctx, case, variable, level, lo, dims, min_level=0, max_level=-1, fill=math.nan,
            with_coverage=True):
    scene = load(ctx, case, variable, min_level, max_level)
    finest = max(b.level for b in scene.all_boxes)
    n_levels = max(level, finest) + 1
    return api.covering_grid_scene(ctx, scene, level, lo, dims, case.sizes()[:n_levels], case.lo,
                                   case.ratio[:n_levels - 1], fill, with_coverage)


def check(ctx, case, level, lo=None, dims=None, min_level=0, max_level=-1, counts=None,
          variables=VARIABLES):
    if lo is None:
        lo, dims = case.whole(level)
    for variable in variables:
        want = case.reference(variable, level, lo, dims, min_level, max_level)
        if counts is not None:          # the case holds every class it is there for
            assert cg.class_counts(want) == counts
        same_grid(grid_of(ctx, case, variable, level, lo, dims, min_level, max_level), want)
    return want


def coverages(result):
    found, counts = np.unique(result["coverage"], return_counts=True)
    return dict(zip(found.tolist(), counts.tolist()))


# ---- hierarchy -----------------------------------------------------------------------------------

@pytest.mark.parametrize("level, counts", [(0, {0: 480, 1: 69, 2: 27}),
                                           (1, {0: 3840, 1: 668, 2: 100}),
                                           (2, {0: 30720, 1: 5344, 2: 800})])
def test_all_levels_over_the_whole_domain(ctx, three, level, counts):
    want = check(ctx, three, level, counts=counts)
    assert coverages(want) == {1.0: sum(counts.values())}
    if level == 0:
        assert int((want["levels_used"] == 2).sum()) == 23     # level-1 and level-2 leaves mixed


@pytest.mark.parametrize("level, levels, counts, covered", [
    (0, (2, -1), {-1: 549, 2: 27}, {0.0: 549, 0.125: 2, 0.25: 9, 0.5: 12, 1.0: 4}),
    (0, (1, -1), {-1: 480, 1: 69, 2: 27}, {0.0: 480, 1.0: 96}),
    (1, (0, 0), {0: 4608}, {1.0: 4608}),
    (2, (0, 1), {0: 30720, 1: 6144}, {1.0: 36864}),     # a level finer than any loaded
])
def test_level_cuts(ctx, three, level, levels, counts, covered):
    want = check(ctx, three, level, None, None, *levels, counts=counts)
    assert coverages(want) == covered


def test_a_sub_region_from_a_negative_index_across_touching_boxes_past_the_domain(ctx, three):
    lo, dims = (-3, 3, 4), (29, 7, 5)            # i = -3 .. 25 of 0 .. 23, across i = 11 | 12
    want = check(ctx, three, 1, lo, dims)
    assert set(cg.class_counts(want)) == {-1, 0, 1, 2}
    assert (want["level"][:, :, 14:16] == 1).any()            # i = 11 | 12 at level 1


def test_ratio_four(ctx, ratio_four):
    want = check(ctx, ratio_four, 0, counts={0: 88, 1: 8})
    assert int((want["levels_used"] == 1).sum()) == 96       # 64 leaves per averaged cell
    check(ctx, ratio_four, 1, counts={0: 24 * 16 * 16 - 512, 1: 512})
    # level 1 alone, from a region that cuts the fine box and leaves the domain
    check(ctx, ratio_four, 0, (1, -1, 2), (5, 4, 3), 1, -1, variables=["u", "odd"])


def test_long_rows_ragged_tiles_a_lone_cell_and_gaps(ctx, shapes):
    want = check(ctx, shapes, 0)
    counts = cg.class_counts(want)
    assert want["values"].shape == (8, 8, 400) and counts[-1] > 10000 and counts[0] > 6000
    assert want["level"][7, 7, 395] == 0 and want["level"][7, 7, 394] == -1
    check(ctx, shapes, 0, (120, -1, 1), (271, 7, 3), variables=["odd"])


# ---- values --------------------------------------------------------------------------------------

def test_the_fill_value_keeps_its_bits_and_the_values_do_not_need_the_coverage(ctx, three):
    lo, dims = three.whole(0)
    for fill in (-0.0, NAN_PAYLOAD, 7.5):
        want = three.reference("odd", 0, lo, dims, 2, -1, fill)
        got = grid_of(ctx, three, "odd", 0, lo, dims, 2, -1, fill)
        same_grid(got, want)
        absent = got[0][got[2] < 0]
        assert absent.size == 549
        assert (absent.view(np.uint64) == np.array([fill]).view(np.uint64)[0]).all()
        alone = grid_of(ctx, three, "odd", 0, lo, dims, 2, -1, fill, with_coverage=False)
        assert alone[1] is None and alone[2] is None
        assert (alone[0].view(np.uint64) == got[0].view(np.uint64)).all()


def test_a_repeat_gives_equal_bits(ctx, three):
    lo, dims = three.whole(0)
    runs = [grid_of(ctx, three, "odd", 0, lo, dims) for _ in range(2)]
    assert ref.same_bits(runs[0][0], runs[1][0]) and ref.same_bits(runs[0][1], runs[1][1])
    assert np.array_equal(runs[0][2], runs[1][2])


# ---- the C ABI -------------------------------------------------------------------------------------

def test_wrong_arguments_are_refused_and_the_outputs_untouched(ctx, three):
    f = load(ctx, three, "u")
    field = ctx.create_scene(f.local_boxes, f.scalar_transform)
    elsewhere = runtime.Context(0)
    foreign = elsewhere.create_scene(f.local_boxes, f.scalar_transform)
    lo, dims = three.whole(0)
    want = three.reference("u", 0, lo, dims)
    shape = want["values"].shape
    values = torch.full(shape, 0.5, dtype=torch.float64, device=ctx.device)
    coverage = torch.full(shape, 0.25, dtype=torch.float64, device=ctx.device)
    levels = torch.full(shape, 7, dtype=torch.int8, device=ctx.device)
    _, _, index = api._level_setup(f, f.local_boxes, three.sizes(), three.lo, three.ratio)
    index = np.ascontiguousarray(index, np.int32)

    def untouched():
        ctx.synchronize()
        return bool((values == 0.5).all()) and bool((coverage == 0.25).all()) and \
            bool((levels == 7).all())

    def call(scene=field, level=0, lo=lo, dims=dims, index=index, ratio=(2, 2), n_levels=3,
             fill=math.nan, values=values, coverage=coverage, levels=levels):
        ints = lambda a: np.ascontiguousarray(a, np.int32)
        lo, dims, index, ratio = ints(lo), ints(dims), ints(index), ints(ratio)
        pointer = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        as_ints = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        return _capi.lib().avr_scene_covering_grid(
            ctx._handle, scene._handle, level, as_ints(lo), as_ints(dims), as_ints(index),
            as_ints(ratio), n_levels, fill, pointer(values), pointer(coverage), pointer(levels))

    overlapping = index.copy()
    same_level = [b for b, box in enumerate(f.local_boxes) if box.level == 1]
    overlapping[same_level[1]] = index[same_level[0]]
    far = index.copy()
    far[0, 0] = 2 ** 30
    inside = f.local_boxes[1].values          # an output array that is an input box's cells
    wrong = [
        (dict(values=inside), "an output array overlaps an input box's cells"),
        (dict(coverage=inside), "an output array overlaps an input box's cells"),
        (dict(levels=inside), "an output array overlaps an input box's cells"),
        (dict(level=3), "level must lie in [0, n_levels)"),                  # level == n_levels
        (dict(level=-1), "level must lie in [0, n_levels)"),
        (dict(dims=(12, 0, 8)), "dims must be at least 1"),
        (dict(dims=(0, 6, 8)), "dims must be at least 1"),
        (dict(scene=foreign),
         "the scenes must belong to the context and hold the same number of boxes"),
        (dict(values=None), "null argument"),
        (dict(n_levels=0), "n_levels must lie in [1, 16]"),
        (dict(n_levels=17, ratio=[2] * 16), "n_levels must lie in [1, 16]"),
        (dict(n_levels=2, ratio=(2,)), "a box's level is not below n_levels"),
        (dict(ratio=(2, 1)), "a level ratio is below 2"),
        (dict(index=far), "a box's index range leaves [-2^30, 2^30)"),
        (dict(index=overlapping), "two boxes of one level overlap in index space"),
        (dict(lo=(2 ** 28, 0, 0)),
         "the region leaves [-2^30, 2^30) at its level or at the finest loaded one"),
        (dict(dims=(2048, 1024, 1024)), "the region has 2^31 cells or more"),
    ]
    for arguments, message in wrong:
        assert call(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert _capi.lib().avr_last_error().decode() == message, arguments
        assert untouched(), arguments
    # ... and the call that is in order writes everything
    assert call() == 0
    ctx.synchronize()
    same_grid((values.cpu().numpy(), coverage.cpu().numpy(), levels.cpu().numpy()), want)
    foreign.close()
    field.close()
    elsewhere.close()


# ---- composition -----------------------------------------------------------------------------------

def regridded(case, dense):
    dlo = [lev["domain"][0] for lev in case.levels]
    cut = lambda l, lo, hi: dense[l][lo[2] - dlo[l][2]:hi[2] - dlo[l][2] + 1,
                                     lo[1] - dlo[l][1]:hi[1] - dlo[l][1] + 1,
                                     lo[0] - dlo[l][0]:hi[0] - dlo[l][0] + 1]
    return [{"domain": lev["domain"], "boxes": lev["boxes"],
             "data": [cut(l, *box)[None] for box in lev["boxes"]]}
            for l, lev in enumerate(case.levels)]


def test_api_covering_grid_of_a_stored_a_derived_and_a_gradient_field(ctx, three, tmp_path):
    out = str(tmp_path / "grid.npz")
    got = api.covering_grid(three.path, 0, ["u", "whole"], output=out)
    lo, dims = three.whole(0)
    want = three.reference("u", 0, lo, dims)
    assert got["level"] == 0 and got["lo"] == lo and got["dims"] == dims
    assert got["left_edge"] == three.lo and got["right_edge"] == three.hi
    assert got["cell_size"] == three.sizes()[0] and list(got["fields"]) == ["u", "whole"]
    same_grid((got["fields"]["u"], got["coverage"], got["cell_level"]), want)
    assert ref.same_bits(got["fields"]["whole"], three.reference("whole", 0, lo, dims)["values"])
    assert got["absent"] == 0 and got["partial"] == 0
    back = grids.load_npz(out)
    assert set(back) == set(got) and list(back["fields"]) == ["u", "whole"]
    for key in ("level", "lo", "dims", "left_edge", "right_edge", "cell_size", "absent", "partial"):
        assert back[key] == got[key], key
    for name in ("u", "whole"):
        assert ref.same_bits(back["fields"][name], got["fields"][name])
    assert ref.same_bits(back["coverage"], got["coverage"])
    assert np.array_equal(back["cell_level"], got["cell_level"])

    # the defaults: the first variable at the finest loaded level; absent and partial cells
    cut = api.covering_grid(three.path, 0, min_level=2)
    want = three.reference("u", 0, lo, dims, 2, -1)
    same_grid((cut["fields"]["u"], cut["coverage"], cut["cell_level"]), want)
    assert cut["absent"] == 549 == int((want["coverage"] == 0.0).sum())
    assert cut["partial"] == 23 == int(((want["coverage"] > 0.0) & (want["coverage"] < 1.0)).sum())
    finest = api.covering_grid(three.path, max_level=1, fields=["odd"])
    lo1, dims1 = three.whole(1)
    assert finest["level"] == 1 and finest["dims"] == dims1
    same_grid((finest["fields"]["odd"], finest["coverage"], finest["cell_level"]),
              three.reference("odd", 1, lo1, dims1, 0, 1))

    # edges against the equivalent region: a range that leaves the domain at level 1
    region = ((-2, 1, 3), (25, 9, 8))
    size = three.sizes()[1]
    left = tuple(three.lo[a] + region[0][a] * size[a] for a in range(3))
    right = tuple(three.lo[a] + (region[1][a] + 1) * size[a] for a in range(3))
    by_index = api.covering_grid(three.path, 1, ["odd"], region=region)
    by_edges = api.covering_grid(three.path, 1, ["odd"], left_edge=left, right_edge=right)
    assert by_index["lo"] == by_edges["lo"] == region[0] and by_index["dims"] == (28, 9, 6)
    assert by_edges["dims"] == by_index["dims"] and by_edges["left_edge"] == left
    assert by_edges["right_edge"] == right == by_index["right_edge"]
    want = three.reference("odd", 1, region[0], (28, 9, 6))
    for found in (by_index, by_edges):
        same_grid((found["fields"]["odd"], found["coverage"], found["cell_level"]), want)
        assert found["absent"] == int((want["coverage"] == 0.0).sum()) > 0

    api.add_field("uu", "u * u")
    squared = derive_reference.evaluate_levels("u * u", three.levels, VARIABLES, three.lo, three.hi)
    levels = [{"domain": lev["domain"], "boxes": lev["boxes"], "data": [g[None] for g in grids_]}
              for lev, grids_ in zip(three.levels, squared)]
    want = cg.covering_grid(levels, three.ratio, 0, 0, lo, dims)
    got = api.covering_grid(three.path, 0, ["uu"])
    same_grid((got["fields"]["uu"], got["coverage"], got["cell_level"]), want)

    api.add_gradient_field("du_dx", "u", "x")
    gradient = ref.gradient_levels(three.levels, three.ratio, three.sizes(), 0, 0)[0]
    want = cg.covering_grid(regridded(three, gradient), three.ratio, 0, 0, lo, dims)
    got = api.covering_grid(three.path, 0, ["du_dx", "u"])
    same_grid((got["fields"]["du_dx"], got["coverage"], got["cell_level"]), want)
    assert ref.same_bits(got["fields"]["u"], three.reference("u", 0, lo, dims)["values"])


def test_a_slice_of_a_stored_variable_is_unchanged_around_a_covering_grid(ctx, three):
    before = api.slice(three.path, 40, 30, "u", axis="y")
    assert api.covering_grid(three.path, 1, ["odd"])["absent"] == 0
    after = api.slice(three.path, 40, 30, "u", axis="y")
    assert ref.same_bits(before, after)
