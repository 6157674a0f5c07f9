"""Grid fields on the GPU: the kernel of avr_grid_field.hip through avr_scene_grid_field,
Scene.grid_field and api.grid_scene, and the registry of gridfields.py through the plotfile-level
functions, against the numpy reference on the plotfile's own level arrays (grid_field_reference).
Values are equal by bits (a NaN equal to a NaN; the fill value by its very bits), the totals are
equal.  Every coarse cell that a finer grid covers holds 1e30 in the plotfile: a box written past
its view would show in the neighbouring box."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, plotfile, runtime
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform

import covering_grid_reference as cg
import gradient_reference as ref
import grid_field_reference as gf

pytestmark = pytest.mark.gpu
VARIABLES = list(ref.VARIABLES)
NAN_PAYLOAD = float(np.array([0x7ff8000000001234], dtype=np.uint64).view(np.float64)[0])
MODES = ("constant", "linear")


@pytest.fixture(autouse=True)
def _empty_registries():
    def clear():
        for name in list(api.grid_fields()):
            api.remove_grid_field(name)
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

    def scene_boxes(self, min_level=0, max_level=-1):
        """(level, lo, hi) of every scene box, in the loader's order."""
        if max_level < 0:
            max_level = len(self.levels) - 1
        convex = plotfile.convexify([lev["boxes"] for lev in self.levels[:max_level + 1]],
                                    self.ratio[:max_level])
        return [(l, lo, hi) for l in range(min_level, max_level + 1) for _, (lo, hi) in convex[l]]

    def cut(self, dense, level, lo, hi):
        dlo = self.levels[level]["domain"][0]
        return dense[level][lo[2] - dlo[2]:hi[2] - dlo[2] + 1, lo[1] - dlo[1]:hi[1] - dlo[1] + 1,
                            lo[0] - dlo[0]:hi[0] - dlo[0] + 1]

    def arrays(self, variable="u", min_level=0, max_level=-1):
        return ref.leaf_arrays(self.levels, self.ratio, VARIABLES.index(variable), min_level,
                               max_level)[0]


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
    return _write(tmp_path_factory.mktemp("gridfield") / "three", THREE_DOMAINS, THREE_BOXES,
                  (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 2], 71)


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    grids_ = [((0, 0, 0), (130, 4, 2)), ((131, 0, 0), (386, 3, 3)), ((387, 0, 0), (387, 3, 3)),
              ((388, 0, 0), (390, 3, 3)), ((395, 7, 7), (395, 7, 7))]
    return _write(tmp_path_factory.mktemp("gridfield") / "shapes", [((0, 0, 0), (399, 7, 7))],
                  [grids_], (0.0, 0.0, 0.0), (100.0, 2.0, 2.0), [], 72)


@pytest.fixture(scope="module")
def ratio_four(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("gridfield") / "four",
                  [((0, 0, 0), (5, 3, 3)), ((0, 0, 0), (23, 15, 15))],
                  [[((0, 0, 0), (5, 3, 3))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (3.0, 2.0, 2.0), [4], 73)


@pytest.fixture(scope="module")
def flat(tmp_path_factory):
    """One level of 16 x 8 x 8 cells: what the transforms take whole."""
    return _write(tmp_path_factory.mktemp("gridfield") / "flat", [((0, 0, 0), (15, 7, 7))],
                  [[((0, 0, 0), (15, 7, 7))]], (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [], 74)


@pytest.fixture(scope="module")
def patched(tmp_path_factory):
    """The same with one finer patch in its middle."""
    return _write(tmp_path_factory.mktemp("gridfield") / "patched",
                  [((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))],
                  [[((0, 0, 0), (15, 7, 7))], [((8, 4, 4), (19, 11, 9))]],
                  (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [2], 75)


def load(ctx, case, name="u", min_level=0, max_level=-1):
    return plotfile.load_plotfile_geometry(ctx, case.path, name, min_level, max_level, False, True)


def levels_of(case, scene, level):
    """(cell_sizes, prob_lo, ref_ratio) up to the finer of `level` and the finest loaded level."""
    n_levels = max(level, max(b.level for b in scene.all_boxes)) + 1
    return case.sizes()[:n_levels], case.lo, case.ratio[:n_levels - 1]


def random_grid(dims, seed=3):
    return np.random.default_rng(seed).standard_normal(dims[::-1])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def boxes_equal(case, out, dense, min_level=0, max_level=-1, exact=False):
    expected = case.scene_boxes(min_level, max_level)
    assert len(out.local_boxes) == len(out.all_boxes) == len(expected) > 0
    for box, (level, lo, hi) in zip(out.local_boxes, expected):
        assert box.level == level
        assert box.cell_dimensions == tuple(hi[a] - lo[a] + 1 for a in range(3))
        got, want = box.values.cpu().numpy(), case.cut(dense, level, lo, hi)
        assert ref.same_bits(got, want), (level, lo, hi)
        if exact:
            assert np.array_equal(bits(got), bits(want)), (level, lo, hi)


def check(ctx, case, grid, level, lo, interpolation=0, periodic=False, fill=math.nan,
          min_level=0, max_level=-1, exact=False):
    scene = load(ctx, case, "u", min_level, max_level)
    out, outside, partial = api.grid_scene(ctx, scene, grid, level, lo,
                                           *levels_of(case, scene, level), MODES[interpolation],
                                           periodic, fill)
    dense, want_outside, want_partial = gf.grid_scene_of(
        case.arrays("u", min_level, max_level), case.ratio, grid, level, lo, interpolation,
        periodic, fill)
    print("level", level, MODES[interpolation], "periodic" if periodic else "clamped",
          "outside:", outside, want_outside, "partial:", partial, want_partial)
    assert out.world_scale == scene.world_scale
    boxes_equal(case, out, dense, min_level, max_level, exact)
    assert (outside, partial) == (want_outside, want_partial)
    return out, outside, partial


# ---- hierarchy -----------------------------------------------------------------------------------

@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("interpolation", [0, 1])
@pytest.mark.parametrize("level", [0, 1, 2])
def test_three_levels_under_a_grid_of_every_level(ctx, three, level, interpolation, periodic):
    lo, dims = three.whole(level)
    _, outside, partial = check(ctx, three, random_grid(dims), level, lo, interpolation, periodic)
    assert outside == 0 and partial == 0


@pytest.mark.parametrize("interpolation", [0, 1])
def test_a_grid_finer_than_any_loaded_level(ctx, three, interpolation):
    lo, dims = three.whole(2)
    check(ctx, three, random_grid(dims), 2, lo, interpolation, max_level=1)
    check(ctx, three, random_grid(dims), 2, lo, interpolation, max_level=0)


@pytest.mark.parametrize("interpolation", [0, 1])
def test_ratio_four(ctx, ratio_four, interpolation):
    for level in (0, 1):
        lo, dims = ratio_four.whole(level)
        check(ctx, ratio_four, random_grid(dims), level, lo, interpolation, True)
    # a level-1 grid that cuts the coarse cells' footprints: 1 .. 64 children each
    _, outside, partial = check(ctx, ratio_four, random_grid((13, 9, 7)), 1, (3, -2, 5),
                                interpolation)
    assert outside > 0 and partial > 0


def test_long_rows_ragged_tiles_a_lone_cell_and_gaps(ctx, shapes):
    lo, dims = shapes.whole(0)
    check(ctx, shapes, random_grid(dims), 0, lo)
    _, outside, _ = check(ctx, shapes, random_grid((271, 7, 3)), 0, (120, -1, 1), 1, True)
    assert outside > 1000


def test_a_sub_region_from_a_negative_index_that_leaves_the_domain(ctx, three):
    grid = random_grid((29, 7, 5))
    for interpolation in (0, 1):
        for periodic in (False, True):
            _, outside, partial = check(ctx, three, grid, 1, (-3, 3, 4), interpolation, periodic)
            assert outside > 500 and partial > 10


# ---- values --------------------------------------------------------------------------------------

def test_the_fill_value_keeps_its_bits(ctx, three):
    grid = random_grid((29, 7, 5))
    for fill in (-0.0, NAN_PAYLOAD, 7.5):
        out, outside, _ = check(ctx, three, grid, 1, (-3, 3, 4), 1, False, fill, exact=fill == fill)
        got = np.concatenate([bits(b.values.cpu().numpy()).reshape(-1) for b in out.local_boxes])
        assert int((got == bits(np.array([fill]))[0]).sum()) == outside


def test_a_grid_with_a_nan_and_both_infinities(ctx, three):
    lo, dims = three.whole(1)
    grid = random_grid(dims).reshape(-1)
    pick = np.random.default_rng(9).choice(grid.size, grid.size // 20, replace=False)
    grid[pick] = np.array([np.nan, np.inf, -np.inf])[np.arange(pick.size) % 3]
    grid = grid.reshape(dims[::-1])
    for interpolation in (0, 1):
        out, _, _ = check(ctx, three, grid, 1, lo, interpolation, True)
        values = np.concatenate([b.values.cpu().numpy().reshape(-1) for b in out.local_boxes])
        assert np.isnan(values).any() and np.isposinf(values).any() and np.isneginf(values).any()


def test_a_repeat_gives_equal_bits(ctx, three):
    lo, dims = three.whole(0)
    runs = [check(ctx, three, random_grid(dims), 0, lo, 1, True)[0] for _ in range(2)]
    for a, b in zip(runs[0].local_boxes, runs[1].local_boxes):
        assert np.array_equal(bits(a.values.cpu().numpy()), bits(b.values.cpu().numpy()))


# ---- Scene.grid_field ----------------------------------------------------------------------------

def native_setup(ctx, case, level):
    scene = load(ctx, case)
    sizes, _, ratio = levels_of(case, scene, level)
    _, ratios, index = api._level_setup(scene, scene.local_boxes, sizes, case.lo, ratio)
    return scene, np.ascontiguousarray(index, np.int32), ratios


@pytest.mark.parametrize("pad", [1, 2])
def test_strided_output_views_take_both_store_widths(ctx, three, pad):
    """Boxes that are views into wider allocations: with a pad of 1 the row stride of an even box
    is odd (single stores), with 2 it is even (pair stores); what lies past a view stays."""
    scene, index, ratios = native_setup(ctx, three, 1)
    lo, dims = three.whole(1)
    grid = random_grid(dims)
    dense, _, _ = gf.grid_scene_of(three.arrays(), three.ratio, grid, 1, lo, 1, False)
    whole, views = [], []
    for b in scene.local_boxes:
        nx, ny, nz = b.cell_dimensions
        wide = torch.full((nz + 1, ny + pad, nx + pad), 0.5, dtype=torch.float64, device=ctx.device)
        whole.append(wide)
        views.append(AmrBox(b.min_corner, b.max_corner, wide[:nz, :ny, :nx], b.level))
    paired = [v.values.data_ptr() % 16 == 0 and v.values.stride(1) % 2 == 0 and
              v.values.stride(0) % 2 == 0 for v in views]
    assert any(paired) if pad == 2 else not all(paired)
    out = ctx.create_scene(views, ScalarTransform())
    totals = out.grid_field(torch.from_numpy(grid).to(ctx.device), 1, lo, index, ratios, 1, False)
    ctx.synchronize()
    assert totals.tolist() == [0, 0]
    for wide, view, (level, blo, bhi) in zip(whole, views, three.scene_boxes()):
        nx, ny, nz = view.cell_dimensions
        assert ref.same_bits(view.values.cpu().numpy(), three.cut(dense, level, blo, bhi))
        rest = wide.clone()
        rest[:nz, :ny, :nx] = 0.5
        assert bool((rest == 0.5).all())
    out.close()


def test_prefilled_totals_are_added_into(ctx, three):
    scene, index, ratios = native_setup(ctx, three, 1)
    grid = random_grid((29, 7, 5))
    _, outside, partial = gf.grid_scene_of(three.arrays(), three.ratio, grid, 1, (-3, 3, 4))
    written = api._blank_like(ctx, scene, 0)
    out = ctx.create_scene(written.local_boxes, ScalarTransform())
    totals = torch.tensor([5, 700], dtype=torch.int64, device=ctx.device)
    device_grid = torch.from_numpy(grid).to(ctx.device)
    for _ in range(2):
        assert out.grid_field(device_grid, 1, (-3, 3, 4), index, ratios, totals=totals) is totals
    ctx.synchronize()
    assert totals.tolist() == [5 + 2 * outside, 700 + 2 * partial]
    out.close()


def test_the_round_trips_through_the_covering_grid(ctx, three):
    """covering_grid -> grid_field gives the field back on every leaf (the integers of `whole`
    leave the means exact); grid_field -> covering_grid gives the grid back wherever the leaves
    are as fine as the grid (a grid of integers, so that the mean of the R^3 copies a finer leaf
    level holds is exact too)."""
    scene = load(ctx, three, "whole")
    sizes, prob_lo, ratio = levels_of(three, scene, 2)
    lo, dims = three.whole(2)
    grid, _, _ = api.covering_grid_scene(ctx, scene, 2, lo, dims, sizes, prob_lo, ratio)
    back, outside, partial = api.grid_scene(ctx, scene, grid, 2, lo, sizes, prob_lo, ratio)
    assert outside == 0 and partial == 0
    for a, b in zip(scene.local_boxes, back.local_boxes):
        assert np.array_equal(bits(a.values.cpu().numpy()), bits(b.values.cpu().numpy()))
    for level in (0, 1, 2):
        lo, dims = three.whole(level)
        grid = np.random.default_rng(11).integers(-1000, 1001, size=dims[::-1]).astype(np.float64)
        out, _, _ = api.grid_scene(ctx, scene, grid, level, lo, sizes, prob_lo, ratio)
        values, _, cell_level = api.covering_grid_scene(ctx, out, level, lo, dims, sizes, prob_lo,
                                                        ratio)
        fine = cell_level >= level
        assert fine.any() and np.array_equal(bits(values[fine]), bits(grid[fine]))


def test_wrong_arguments_are_refused_and_the_outputs_untouched(ctx, three):
    scene, index, _ = native_setup(ctx, three, 0)
    written = api._blank_like(ctx, scene, 0)
    for box in written.local_boxes:
        box.values.fill_(0.5)
    out = ctx.create_scene(written.local_boxes, ScalarTransform())
    elsewhere = runtime.Context(0)
    foreign = elsewhere.create_scene(written.local_boxes, ScalarTransform())
    lo, dims = three.whole(0)
    grid = torch.from_numpy(random_grid(dims)).to(ctx.device)
    totals = torch.tensor([3, 4], dtype=torch.int64, device=ctx.device)

    def untouched():
        ctx.synchronize()
        return totals.tolist() == [3, 4] and \
            all(bool((b.values == 0.5).all()) for b in written.local_boxes)

    def call(scene=out, grid=grid, level=0, lo=lo, dims=dims, index=index, ratio=(2, 2),
             n_levels=3, interpolation=0, periodic=0, fill=math.nan, totals=totals):
        ints = lambda a: np.ascontiguousarray(a, np.int32)
        lo, dims, index, ratio = ints(lo), ints(dims), ints(index), ints(ratio)
        pointer = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        as_ints = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        return _capi.lib().avr_scene_grid_field(
            ctx._handle, scene._handle, pointer(grid), level, as_ints(lo), as_ints(dims),
            as_ints(index), as_ints(ratio), n_levels, interpolation, periodic, fill,
            pointer(totals))

    far = index.copy()
    far[0, 0] = 2 ** 30
    inside = written.local_boxes[1].values          # a grid that is an output box's cells
    shared = "the grid or the totals overlap an output box's cells"
    wrong = [
        (dict(grid=inside), shared),
        (dict(totals=inside.view(torch.int64)), shared),
        (dict(level=3), "level must lie in [0, n_levels)"),
        (dict(level=-1), "level must lie in [0, n_levels)"),
        (dict(dims=(12, 0, 8)), "dims must be at least 1"),
        (dict(scene=foreign),
         "the scenes must belong to the context and hold the same number of boxes"),
        (dict(grid=None), "null argument"),
        (dict(totals=None), "null argument"),
        (dict(n_levels=0), "n_levels must lie in [1, 16]"),
        (dict(n_levels=17, ratio=[2] * 16), "n_levels must lie in [1, 16]"),
        (dict(n_levels=2, ratio=(2,)), "a box's level is not below n_levels"),
        (dict(ratio=(2, 1)), "a level ratio is below 2"),
        (dict(index=far), "a box's index range leaves [-2^30, 2^30)"),
        (dict(lo=(2 ** 28, 0, 0)),
         "the region leaves [-2^30, 2^30) at its level or at the finest box level"),
        (dict(dims=(2048, 1024, 1024)), "the region has 2^31 cells or more"),
        (dict(interpolation=2), "interpolation must be 0 (constant) or 1 (linear)"),
        (dict(periodic=2), "periodic must be 0 or 1"),
    ]
    for arguments, message in wrong:
        assert call(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert _capi.lib().avr_last_error().decode() == message, arguments
        assert untouched(), arguments
    # ... and the call that is in order writes everything
    assert call() == 0
    ctx.synchronize()
    dense, _, _ = gf.grid_scene_of(three.arrays(), three.ratio, grid.cpu().numpy(), 0, lo)
    boxes_equal(three, written, dense)
    assert totals.tolist() == [3, 4]
    foreign.close()
    out.close()
    elsewhere.close()


# ---- the registry through the plotfile-level functions ---------------------------------------------

def field_grid(path, name, level=0):
    return api.covering_grid(path, level, [name])["fields"][name]


def test_on_one_level_a_grid_field_is_the_products_own_grid(ctx, flat):
    api.add_potential_field("phi", "u", constant=2.5)
    api.add_potential_field("phi_open", "u", constant=2.5, boundary="isolated", self_term=1.5)
    api.add_field("uu", "u * u")
    velocity = ("u", "whole", "uu")
    api.add_helmholtz_field("sol_y", velocity, "solenoidal", "y")
    api.add_helmholtz_field("comp_x", velocity, "compressive", "x")
    want = api.potential(flat.path, "u", 2.5)["potential"]
    assert np.array_equal(bits(field_grid(flat.path, "phi")), bits(want))
    want = api.isolated_potential(flat.path, "u", 2.5, self_term=1.5)["potential"]
    assert np.array_equal(bits(field_grid(flat.path, "phi_open")), bits(want))
    split = api.helmholtz(flat.path, velocity)
    got = api.covering_grid(flat.path, 0, ["sol_y", "comp_x"])["fields"]      # one split for both
    assert np.array_equal(bits(got["sol_y"]), bits(split["solenoidal"]["whole"]))
    assert np.array_equal(bits(got["comp_x"]), bits(split["compressive"]["u"]))


@pytest.mark.parametrize("interpolation", MODES)
def test_with_a_finer_patch_a_grid_field_is_the_reference_on_the_products_grid(ctx, patched,
                                                                                interpolation):
    api.add_potential_field("phi", "u", level=0, interpolation=interpolation)
    grid = api.potential(patched.path, "u", level=0)["potential"]
    dense, _, _ = gf.grid_scene_of(patched.arrays(), patched.ratio, grid, 0, (0, 0, 0),
                                   MODES.index(interpolation), True)
    _, _, _, _, scenes, _ = api._load_fields(patched.path, ["phi"], 0, -1)
    boxes_equal(patched, scenes[0], dense)
    # level None: the finest loaded level, whose grid the coarse leaves average
    api.add_potential_field("phi_fine", "u", interpolation=interpolation)
    grid = api.potential(patched.path, "u")["potential"]
    assert grid.shape == (16, 16, 32)
    dense, _, _ = gf.grid_scene_of(patched.arrays(), patched.ratio, grid, 1, (0, 0, 0),
                                   MODES.index(interpolation), True)
    _, _, _, _, scenes, _ = api._load_fields(patched.path, ["phi_fine"], 0, -1)
    boxes_equal(patched, scenes[0], dense)


def test_a_derived_field_reads_a_grid_field(ctx, patched):
    lo, dims = patched.whole(0)
    grid = random_grid(dims, 21)
    api.add_array_field("g", grid, 0)
    api.add_field("e_grav", "0.5 * u * g")
    written, _, _ = gf.grid_scene_of(patched.arrays(), patched.ratio, grid, 0, lo)
    dense = [(0.5 * values) * g for (_, _, values), g in zip(patched.arrays(), written)]
    _, _, _, _, scenes, _ = api._load_fields(patched.path, ["e_grav"], 0, -1)
    boxes_equal(patched, scenes[0], dense)


def test_a_grid_field_through_slice_profile_and_clumps_equals_the_array_of_its_grid(ctx, patched):
    api.add_potential_field("phi", "u", level=0)
    grid = api.potential(patched.path, "u", level=0)["potential"]
    api.add_array_field("phi_array", grid, 0, interpolation="linear", periodic=True)
    a = api.slice(patched.path, 40, 30, "phi", axis="z")
    b = api.slice(patched.path, 40, 30, "phi_array", axis="z")
    assert ref.same_bits(a, b)
    a = api.profile(patched.path, "phi", "u", bins=8)
    b = api.profile(patched.path, "phi_array", "u", bins=8)
    assert ref.same_bits(a["x_edges"], b["x_edges"])
    assert np.array_equal(a["cells"], b["cells"]) and int(a["cells"].sum()) > 0
    # the histogram adds a bin's n values in no fixed order: each run's weighted sum lies within
    # (n - 1) roundings of 2^-53 of sum |w y|, its mean within that of max |y|; two runs, and the
    # few roundings of the sum over the levels and of the division
    largest = max(float(np.abs(values[mask]).max()) for _, mask, values in patched.arrays())
    bound = 2.0 * (a["cells"] + 4) * 2.0 ** -53 * largest
    assert (np.abs(a["mean"] - b["mean"]) <= bound).all()
    threshold = float(np.median(grid))
    a = api.clumps(patched.path, "phi", upper=threshold)
    b = api.clumps(patched.path, "phi_array", upper=threshold)
    assert a["n"] == b["n"] >= 1 and np.array_equal(a["cells"], b["cells"])


def test_products_of_stored_variables_are_unchanged_around_a_grid_field(ctx, patched):
    before = api.slice(patched.path, 40, 30, "u", axis="y")
    api.add_potential_field("phi", "u")
    assert np.isfinite(api.slice(patched.path, 40, 30, "phi", axis="y")).any()
    after = api.slice(patched.path, 40, 30, "u", axis="y")
    assert ref.same_bits(before, after)
