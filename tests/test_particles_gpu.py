"""Particle fields on the GPU: the kernels of avr_particles.hip through avr_scene_particle_cells and
avr_scene_particle_deposit, Scene.particle_cells / particle_deposit and api.deposit_scene, and the
registry of particles.py through the plotfile-level functions, against the numpy reference on the
plotfile's own level arrays (particle_reference).  Cells, shares, levels and deposited values are
equal by bits (a NaN equal to a NaN), the counts are equal; there is no tolerance anywhere."""
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
import particle_reference as pr

pytestmark = pytest.mark.gpu
VARIABLES = list(ref.VARIABLES)
OUTSIDE = 0xFFFFFFFF
SENTINEL = float(np.array([0x7ff8000000001234], dtype=np.uint64).view(np.float64)[0])
METHODS = ("ngp", "cic")
QUANTITIES = ("sum", "density")


def clear_registries():
    for names, remove in ((api.particle_fields, api.remove_particle_field),
                          (api.grid_fields, api.remove_grid_field),
                          (api.clump_fields, api.remove_clump_field),
                          (api.gradient_fields, api.remove_gradient_field),
                          (api.derived_fields, api.remove_field)):
        for name in list(names()):
            remove(name)


@pytest.fixture(autouse=True)
def _empty_registries():
    clear_registries()
    yield
    clear_registries()


@dataclasses.dataclass(eq=False)
class Case:
    path: str
    levels: list
    lo: tuple
    hi: tuple
    ratio: list

    def sizes(self):
        return ref.cell_sizes(self.levels, self.lo, self.hi)

    def hierarchy(self, min_level=0, max_level=-1):
        return pr.hierarchy(self.levels, self.ratio, self.sizes(), self.lo, min_level, max_level)

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

    def ordinals(self, min_level=0, max_level=-1):
        """Per level the cell ordinal of "Clumps" over the level's domain, -1 where no scene box
        holds the cell: the cells of the boxes in scene order, (k ny + j) nx + i inside a box."""
        maps = [np.full(tuple(lev["domain"][1][a] - lev["domain"][0][a] + 1 for a in (2, 1, 0)),
                        -1, dtype=np.int64) for lev in self.levels]
        begin = 0
        for level, lo, hi in self.scene_boxes(min_level, max_level):
            view = self.cut(maps, level, lo, hi)
            view[...] = begin + np.arange(view.size).reshape(view.shape)
            begin += view.size
        return maps


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
    return _write(tmp_path_factory.mktemp("particles") / "three", THREE_DOMAINS, THREE_BOXES,
                  (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 2], 71)


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    grids_ = [((0, 0, 0), (130, 4, 2)), ((131, 0, 0), (386, 3, 3)), ((387, 0, 0), (387, 3, 3)),
              ((388, 0, 0), (390, 3, 3)), ((395, 7, 7), (395, 7, 7))]
    return _write(tmp_path_factory.mktemp("particles") / "shapes", [((0, 0, 0), (399, 7, 7))],
                  [grids_], (0.0, 0.0, 0.0), (100.0, 2.0, 2.0), [], 72)


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    """72 boxes of one column of cells each: the locator's lists and the ordinal prefix."""
    grids_ = [((i, 0, 0), (i, 3, 3)) for i in range(72)]
    return _write(tmp_path_factory.mktemp("particles") / "many", [((0, 0, 0), (71, 3, 3))],
                  [grids_], (0.0, 0.0, 0.0), (18.0, 1.0, 1.0), [], 76)


@pytest.fixture(scope="module")
def ratio_four(tmp_path_factory):
    return _write(tmp_path_factory.mktemp("particles") / "four",
                  [((0, 0, 0), (5, 3, 3)), ((0, 0, 0), (23, 15, 15))],
                  [[((0, 0, 0), (5, 3, 3))], [((8, 4, 4), (15, 11, 11))]],
                  (0.0, 0.0, 0.0), (3.0, 2.0, 2.0), [4], 73)


@pytest.fixture(scope="module")
def flat(tmp_path_factory):
    """One level of 16 x 8 x 8 cells."""
    return _write(tmp_path_factory.mktemp("particles") / "flat", [((0, 0, 0), (15, 7, 7))],
                  [[((0, 0, 0), (15, 7, 7))]], (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [], 74)


@pytest.fixture(scope="module")
def patched(tmp_path_factory):
    """The same with one finer patch in its middle."""
    return _write(tmp_path_factory.mktemp("particles") / "patched",
                  [((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))],
                  [[((0, 0, 0), (15, 7, 7))], [((8, 4, 4), (19, 11, 9))]],
                  (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [2], 75)


def load(ctx, case, min_level=0, max_level=-1):
    return plotfile.load_plotfile_geometry(ctx, case.path, "u", min_level, max_level, False, True)


def levels_of(case, scene):
    n_levels = max(b.level for b in scene.all_boxes) + 1
    return case.sizes()[:n_levels], case.lo, case.ratio[:n_levels - 1]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(got, want):
    """Equal by bits, a NaN equal to a NaN."""
    return ref.same_bits(got, want)


def random_particles(case, n, seed, odd=True):
    """n particles over a little more than the domain, about 2 % of the values NaN or +-Inf."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(case.lo), np.array(case.hi)
    points = lo - 0.02 * (hi - lo) + rng.random((n, 3)) * 1.04 * (hi - lo)
    values = rng.standard_normal(n)
    if odd and n:
        pick = rng.choice(n, max(n // 50, min(n, 3)), replace=False)
        values[pick] = np.array([np.nan, np.inf, -np.inf])[np.arange(pick.size) % 3]
    return points, values


def special_positions(case, min_level=0, max_level=-1):
    """On, one ulp off and within half a cell of every face of every scene box (cell faces, box
    faces, coarse-fine faces, the hole's and the domain's faces, prob_hi exactly), and positions
    that are no number."""
    rng = np.random.default_rng(17)
    sizes, lo0 = case.sizes(), np.array(case.lo)
    points = [list(case.hi), list(case.lo), [math.nan, 0.1, 2.5], [0.1, math.inf, 2.5],
              [0.1, 0.1, -math.inf], [1e300, 0.0, 2.5], [-1e300, 0.0, 2.5]]
    for level, lo, hi in case.scene_boxes(min_level, max_level):
        dx = np.array(sizes[level])
        for axis in range(3):
            for face in (lo[axis], hi[axis] + 1, lo[axis] + 1):
                at = lo0[axis] + face * dx[axis]
                for offset in (0.0, None, -dx[axis] / 4, dx[axis] / 4, -0.49 * dx[axis],
                               0.49 * dx[axis], -dx[axis] / 2, dx[axis] / 2):
                    p = lo0 + (np.array(lo) + rng.random(3) * (np.array(hi) - lo + 1)) * dx
                    if offset is None:
                        for towards in (-math.inf, math.inf):
                            q = p.copy()
                            q[axis] = np.nextafter(at, towards)
                            points.append(q.tolist())
                        continue
                    p[axis] = at + offset
                    points.append(p.tolist())
    return np.array(points, dtype=np.float64)


def expected_cells(case, found, min_level=0, max_level=-1):
    maps = case.ordinals(min_level, max_level)
    level, index = found["level"], found["index"]
    out = np.full(level.shape, OUTSIDE, dtype=np.int64)
    for l, lev in enumerate(case.levels):
        pick = level == l
        rel = index[pick] - np.array(lev["domain"][0])[None, :]
        out[pick] = maps[l][rel[:, 2], rel[:, 1], rel[:, 0]]
    assert (out >= 0).all()
    return out


def boxes_equal(case, out, dense, min_level=0, max_level=-1, exact=True):
    expected = case.scene_boxes(min_level, max_level)
    assert len(out.local_boxes) == len(out.all_boxes) == len(expected) > 0
    for box, (level, lo, hi) in zip(out.local_boxes, expected):
        assert box.level == level
        got, want = box.values.cpu().numpy(), case.cut(dense, level, lo, hi)
        assert same(got, want), (level, lo, hi)
        if exact:       # +0.0 by its bits where nothing lands
            numbers = ~np.isnan(want)
            assert np.array_equal(bits(got)[numbers], bits(want)[numbers]), (level, lo, hi)


def native_setup(ctx, case, min_level=0, max_level=-1):
    scene = load(ctx, case, min_level, max_level)
    sizes, prob_lo, ratio = levels_of(case, scene)
    sizes, ratios, index = api._level_setup(scene, scene.local_boxes, sizes, prob_lo, ratio)
    return scene, np.ascontiguousarray(index, np.int32), ratios, sizes


def check_cells(ctx, case, points, values, method, min_level=0, max_level=-1):
    """Cells, shares, levels and totals before any sort, then the deposited scene of both
    quantities, against the reference."""
    scene, index, ratios, sizes = native_setup(ctx, case, min_level, max_level)
    h = case.hierarchy(min_level, max_level)
    found = pr.contributions(h, points, values, method)
    written = api._blank_like(ctx, scene, 0)
    with api._native_scenes(ctx, [written]) as (out,):
        cells, shares, levels, totals = out.particle_cells(points, values, method, index, ratios,
                                                           sizes, case.lo, levels=True)
        ctx.synchronize()
        print(METHODS[method], "n", len(points), "outside", totals.tolist()[0], found["outside"],
              "rerouted", totals.tolist()[1], found["rerouted"])
        assert totals.tolist() == [found["outside"], found["rerouted"]]
        assert np.array_equal(cells.cpu().numpy(),
                              expected_cells(case, found, min_level, max_level))
        assert same(shares.cpu().numpy(), found["shares"])
        assert np.array_equal(levels.cpu().numpy(),
                              np.where(found["leaf_level"] < 0, 255, found["leaf_level"]))
        for quantity in (0, 1):
            for box in written.local_boxes:
                box.values.fill_(SENTINEL)
            out.particle_deposit(cells, shares, quantity, sizes)
            ctx.synchronize()
            boxes_equal(case, written, pr.deposit(h, found, quantity), min_level, max_level)
    return found


# ---- against the reference -----------------------------------------------------------------------

@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 4096])
def test_random_particles_on_three_levels(ctx, three, n, method):
    points, values = random_particles(three, n, 100 + n)
    found = check_cells(ctx, three, points, values, method)
    if n >= 255:
        assert found["outside"] > 0 and (found["leaf_level"] == 2).any()
        assert method == 0 or found["rerouted"] > 0


@pytest.mark.parametrize("method", [0, 1])
@pytest.mark.parametrize("load_levels", [(0, -1), (1, -1), (0, 0)])
def test_special_positions_at_all_levels_with_a_hole_and_on_one_level(ctx, three, load_levels,
                                                                      method):
    points = special_positions(three, *load_levels)
    extra, _ = random_particles(three, 300, 5, odd=False)       # some of them in the hole
    points = np.concatenate([points, extra])
    values = np.random.default_rng(3).standard_normal(len(points))
    found = check_cells(ctx, three, points, values, method, *load_levels)
    assert found["leaf_level"][0] == -1                         # prob_hi itself
    assert found["outside"] >= 7
    if load_levels[0] == 1:
        assert found["outside"] > 100                           # the hole


@pytest.mark.parametrize("method", [0, 1])
def test_ratio_four(ctx, ratio_four, method):
    points = np.concatenate([special_positions(ratio_four), random_particles(ratio_four, 257, 8)[0]])
    found = check_cells(ctx, ratio_four, points, None, method)
    assert (found["leaf_level"] == 1).any() and (found["leaf_level"] == 0).any()


@pytest.mark.parametrize("method", [0, 1])
def test_long_rows_a_lone_cell_gaps_and_many_boxes(ctx, shapes, many, method):
    for case in (shapes, many):
        assert case is shapes or len(case.scene_boxes()) >= 64
        points = np.concatenate([special_positions(case), random_particles(case, 1000, 9)[0]])
        found = check_cells(ctx, case, points, None, method)
        assert found["outside"] > 0 and (found["leaf_level"] == 0).sum() > 200


# ---- runs ----------------------------------------------------------------------------------------

def test_a_thousand_particles_in_one_cell_and_a_run_from_a_workgroups_last_lane(ctx, three):
    sizes, lo = three.sizes(), np.array(three.lo)
    rng = np.random.default_rng(21)
    cell_a = lo + (np.array([1, 1, 1]) + 0.5) * np.array(sizes[0])       # a level-0 leaf
    cell_b = lo + (np.array([14, 8, 8]) + 0.5) * np.array(sizes[2])      # a level-2 leaf, after it
    # 255 entries of the first cell, then a run of 1000 that begins in lane 255 and crosses three
    # workgroups; interleaved in the list, so that the stable sort has work to do
    which = np.concatenate([np.zeros(255, dtype=int), np.ones(1000, dtype=int)])
    rng.shuffle(which)
    points = np.where(which[:, None] == 0, cell_a[None, :], cell_b[None, :])
    points = points + (rng.random(points.shape) - 0.5) * 0.9 * np.array(sizes[2])[None, :]
    values = rng.standard_normal(len(points)) * 10.0 ** rng.integers(-8, 9, len(points))
    found = check_cells(ctx, three, points, values, 0)
    assert found["outside"] == 0
    assert sorted(np.unique(found["leaf_level"], return_counts=True)[1].tolist()) == [255, 1000]
    check_cells(ctx, three, points, values, 1)


def test_the_order_of_the_list_is_the_order_of_the_sum(ctx, three):
    points, values = random_particles(three, 4001, 33, odd=False)
    at = np.array(three.lo) + (np.array([1, 1, 1]) + 0.5) * np.array(three.sizes()[0])
    h = three.hierarchy()
    level, _, index = h.locate(points)
    keep = ~((level == 0) & (index == np.array([1, 1, 1])).all(axis=1))
    points[~keep] = np.array(three.hi) + 1.0                    # nobody else in that cell
    for method in (0, 1):
        for order, total in (((1e16, 1.0, -1e16), 0.0), ((1e16, -1e16, 1.0), 1.0)):
            points[[0, 2000, 4000]] = at
            values[[0, 2000, 4000]] = order
            scene = load(ctx, three)
            out, _, _ = api.deposit_scene(ctx, scene, points, values, *levels_of(three, scene),
                                          METHODS[method], "sum")
            dense = pr.deposit(h, pr.contributions(h, points, values, method), 0)
            boxes_equal(three, out, dense)
            if method == 0:
                assert dense[0][1, 1, 1] == total


# ---- output handling -----------------------------------------------------------------------------

@pytest.mark.parametrize("pad", [1, 2])
def test_strided_output_views_take_both_store_widths(ctx, three, pad):
    """Boxes that are views into wider allocations: with a pad of 1 the row stride of an even box
    is odd (single stores), with 2 it is even (pair stores); what lies past a view stays."""
    scene, index, ratios, sizes = native_setup(ctx, three)
    points, values = random_particles(three, 3000, 44)
    h = three.hierarchy()
    dense = pr.deposit(h, pr.contributions(h, points, values, 1), 1)
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
    cells, shares, _, _ = out.particle_cells(points, values, 1, index, ratios, sizes, three.lo)
    out.particle_deposit(cells, shares, 1, sizes)
    ctx.synchronize()
    for wide, view, (level, blo, bhi) in zip(whole, views, three.scene_boxes()):
        nx, ny, nz = view.cell_dimensions
        assert same(view.values.cpu().numpy(), three.cut(dense, level, blo, bhi))
        rest = wide.clone()
        rest[:nz, :ny, :nx] = 0.5
        assert bool((rest == 0.5).all())
    out.close()


def test_prefilled_totals_are_added_into_and_a_repeat_gives_equal_bits(ctx, three):
    scene, index, ratios, sizes = native_setup(ctx, three)
    points, values = random_particles(three, 2000, 55)
    found = pr.contributions(three.hierarchy(), points, values, 1)
    out = ctx.create_scene(scene.local_boxes, scene.scalar_transform)
    totals = torch.tensor([5, 700], dtype=torch.int64, device=ctx.device)
    runs = []
    for _ in range(2):
        cells, shares, _, back = out.particle_cells(points, values, 1, index, ratios, sizes,
                                                    three.lo, totals=totals)
        assert back is totals
        runs.append((cells.cpu().numpy(), shares.cpu().numpy()))
    ctx.synchronize()
    assert totals.tolist() == [5 + 2 * found["outside"], 700 + 2 * found["rerouted"]]
    assert np.array_equal(runs[0][0], runs[1][0]) and same(runs[0][1], runs[1][1])
    out.close()


def test_integer_values_on_quarter_cells_are_conserved_exactly(ctx, three):
    rng = np.random.default_rng(66)
    fine = np.array(three.sizes()[2])
    points = np.array(three.lo) + rng.integers(-8, 4 * 48 + 8, size=(3000, 3)) * fine / 4.0
    values = rng.integers(-50, 51, size=3000).astype(np.float64)
    scene = load(ctx, three)
    inside = three.hierarchy().locate(points)[0] >= 0
    for method in METHODS:
        for quantity in QUANTITIES:
            out, outside, rerouted = api.deposit_scene(ctx, scene, points, values,
                                                       *levels_of(three, scene), method, quantity)
            total = 0.0
            for box in out.local_boxes:
                dx = three.sizes()[box.level]
                volume = (dx[0] * dx[1]) * dx[2]
                total += float(box.values.cpu().numpy().sum()) * \
                    (volume if quantity == "density" else 1.0)
            print(method, quantity, "total", total, "outside", outside, "rerouted", rerouted)
            assert total == float(values[inside].sum())
            assert outside == int((~inside).sum()) > 0
            assert (rerouted > 0) == (method == "cic")


# ---- native refusals -----------------------------------------------------------------------------

def test_wrong_arguments_are_refused_and_the_outputs_untouched(ctx, three):
    scene, index, ratios, sizes = native_setup(ctx, three)
    written = api._blank_like(ctx, scene, 0)
    for box in written.local_boxes:
        box.values.fill_(0.5)
    out = ctx.create_scene(written.local_boxes, ScalarTransform())
    elsewhere = runtime.Context(0)
    foreign = elsewhere.create_scene(written.local_boxes, ScalarTransform())
    n = 100
    device = ctx.device
    points = torch.from_numpy(random_particles(three, n, 77)[0]).to(device)
    values = torch.ones(n, dtype=torch.float64, device=device)
    cells = torch.full((n, 8), 7, dtype=torch.int64, device=device)
    shares = torch.full((n, 8), 0.25, dtype=torch.float64, device=device)
    levels = torch.full((n,), 9, dtype=torch.uint8, device=device)
    totals = torch.tensor([3, 4], dtype=torch.int64, device=device)
    ordered = torch.arange(n, dtype=torch.int64, device=device)
    picked = torch.ones(n, dtype=torch.float64, device=device)

    def untouched():
        ctx.synchronize()
        return totals.tolist() == [3, 4] and bool((cells == 7).all()) and \
            bool((shares == 0.25).all()) and bool((levels == 9).all()) and \
            all(bool((b.values == 0.5).all()) for b in written.local_boxes)

    ints = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    doubles = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    pointer = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def locate(scene=out, points=points, n=n, values=values, method=1, index=index, ratio=(2, 2),
               sizes=sizes, prob_lo=three.lo, n_levels=3, cells=cells, shares=shares,
               levels=levels, totals=totals):
        return _capi.lib().avr_scene_particle_cells(
            ctx._handle, scene._handle, pointer(points), n, pointer(values), method, ints(index),
            ints(ratio), doubles(sizes), doubles(prob_lo), n_levels, pointer(cells),
            pointer(shares), pointer(levels), pointer(totals))

    def deposit(scene=out, cells=ordered, shares=picked, n=n, quantity=0, sizes=sizes, n_levels=3):
        return _capi.lib().avr_scene_particle_deposit(
            ctx._handle, scene._handle, pointer(cells), pointer(shares), n, quantity,
            doubles(sizes), n_levels)

    far = index.copy()
    far[0, 0] = 2 ** 30
    overlapping = index.copy()
    overlapping[1] = overlapping[0]
    bad_sizes = np.array(sizes, dtype=np.float64)
    bad_sizes[1, 1] = 0.0
    box_cells = written.local_boxes[1].values
    wrong = [
        (locate, dict(scene=foreign),
         "the scenes must belong to the context and hold the same number of boxes"),
        (locate, dict(n_levels=0), "n_levels must lie in [1, 16]"),
        (locate, dict(n_levels=17), "n_levels must lie in [1, 16]"),
        (locate, dict(points=None), "null argument"),
        (locate, dict(cells=None), "null argument"),
        (locate, dict(shares=None), "null argument"),
        (locate, dict(totals=None), "null argument"),
        (locate, dict(method=2), "method must be 0 (nearest grid point) or 1 (cloud in cell)"),
        (locate, dict(n=2 ** 28), "n must stay below 2^28 for cloud in cell"),
        (locate, dict(n=2 ** 31, method=0), "n must stay below 2^31"),
        (locate, dict(sizes=bad_sizes), "level_cell_size must be finite and positive"),
        (locate, dict(prob_lo=(0.0, math.nan, 0.0)), "prob_lo must be finite"),
        (locate, dict(n_levels=2, ratio=(2,)), "a box's level is not below n_levels"),
        (locate, dict(ratio=(2, 1)), "a level ratio is below 2"),
        (locate, dict(index=far), "a box's index range leaves [-2^30, 2^30)"),
        (locate, dict(index=overlapping), "two boxes of one level overlap in index space"),
        (locate, dict(shares=cells.view(torch.float64)), "two output arrays overlap"),
        (locate, dict(levels=totals.view(torch.uint8)), "two output arrays overlap"),
        (locate, dict(points=shares), "an output array overlaps the points or the values"),
        (locate, dict(values=cells.view(torch.float64)),
         "an output array overlaps the points or the values"),
        (deposit, dict(scene=foreign),
         "the scenes must belong to the context and hold the same number of boxes"),
        (deposit, dict(n_levels=0), "n_levels must lie in [1, 16]"),
        (deposit, dict(cells=None), "null argument"),
        (deposit, dict(shares=None), "null argument"),
        (deposit, dict(quantity=2), "quantity must be 0 (sum) or 1 (density)"),
        (deposit, dict(n=2 ** 31), "n_contributions must stay below 2^31"),
        (deposit, dict(sizes=bad_sizes), "level_cell_size must be finite and positive"),
        (deposit, dict(n_levels=2), "a box's level is not below n_levels"),
        (deposit, dict(cells=box_cells.view(torch.int64)),
         "the cells or the shares overlap an output box's cells"),
        (deposit, dict(shares=box_cells),
         "the cells or the shares overlap an output box's cells"),
    ]
    for call, arguments, message in wrong:
        assert call(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert _capi.lib().avr_last_error().decode() == message, arguments
        assert untouched(), arguments
    # n == 0 launches nothing for the cells, and still clears for the deposit
    assert locate(n=0, points=None, values=None, cells=None, shares=None, levels=None) == 0
    assert untouched()
    assert deposit(n=0, cells=None, shares=None) == 0
    ctx.synchronize()
    for box in written.local_boxes:
        assert np.array_equal(bits(box.values.cpu().numpy()), np.zeros(box.values.shape, np.uint64))
    # ordinals that name no cell are skipped, whatever the order: nothing but the boxes is written
    n_cells = sum(int(b.values.numel()) for b in written.local_boxes)
    stray = torch.tensor([-5, 3, 3, n_cells, OUTSIDE, 2 ** 40, 1], dtype=torch.int64, device=device)
    assert deposit(cells=stray, shares=picked[:7].contiguous(), n=7, quantity=0) == 0
    ctx.synchronize()
    first = written.local_boxes[0].values.cpu().numpy().reshape(-1)
    assert first[3] == 2.0 and first[1] == 1.0 and float(first.sum()) == 3.0
    assert all(not bool(b.values.any()) for b in written.local_boxes[1:])
    # ... and the call that is in order writes everything
    assert locate() == 0 and untouched() is False
    foreign.close()
    out.close()
    elsewhere.close()


# ---- the registry through the plotfile-level functions ---------------------------------------------

def dyadic_particles(case, n, seed):
    """Integer values at multiples of a quarter of the finest cell, some past the domain."""
    rng = np.random.default_rng(seed)
    fine = np.array(case.sizes()[-1])
    cells = [case.levels[-1]["domain"][1][a] + 1 for a in range(3)]
    points = np.array(case.lo) + np.stack(
        [rng.integers(-4, 4 * cells[a] + 4, size=n) for a in range(3)], axis=1) * fine / 4.0
    return points, rng.integers(1, 60, size=n).astype(np.float64)


def reference_arrays(case, points, values, method, quantity):
    """The reference's scene as leaf arrays: (origin, mask, values) per level."""
    h = case.hierarchy()
    dense = pr.deposit(h, pr.contributions(h, points, values, method), quantity)
    return [(h.origin[l], h.mask[l], dense[l]) for l in range(len(dense))], h


@pytest.mark.parametrize("which", ["flat", "patched"])
def test_a_particle_field_through_the_covering_grid_a_projection_and_a_derived_field(
        ctx, flat, patched, which):
    case = flat if which == "flat" else patched
    finest = len(case.levels) - 1
    points, values = dyadic_particles(case, 600, 88)
    api.add_particle_field("stars", points, values)                      # cic, density
    api.add_particle_field("count", points, None, "ngp", "sum")
    api.add_field("both", "u + stars")
    lo, dims = cg.whole_domain(case.levels, case.ratio, finest)
    for name, method, quantity in (("stars", 1, 1), ("count", 0, 0)):
        arrays, h = reference_arrays(case, points, values if name == "stars" else None, method,
                                     quantity)
        want = cg.covering_grid_of(arrays, case.ratio, finest, lo, dims)["values"]
        got = api.covering_grid(case.path, finest, [name])["fields"][name]
        assert np.array_equal(bits(got), bits(want)) and got.any()
    # the surface density, summed times the pixel area, is the mass inside
    inside = h.locate(points)[0] >= 0
    image = api.project_axis(case.path, "z", "stars", width=dims[0], height=dims[1])
    fine = case.sizes()[finest]
    assert float(image.sum()) * (fine[0] * fine[1]) == float(values[inside].sum())
    # a derived field reads it like a stored variable
    arrays, _ = reference_arrays(case, points, values, 1, 1)
    u = ref.leaf_arrays(case.levels, case.ratio, VARIABLES.index("u"))[0]
    dense = [mine[2] + theirs[2] for mine, theirs in zip(u, arrays)]
    _, _, _, _, scenes, _ = api._load_fields(case.path, ["both"], 0, -1)
    boxes_equal(case, scenes[0], dense, exact=False)


def test_a_particle_field_through_slice_and_profile_equals_the_array_of_its_cells(ctx, flat):
    points, values = random_particles(flat, 800, 91, odd=False)
    api.add_particle_field("stars", points, values, "cic", "density")
    arrays, _ = reference_arrays(flat, points, values, 1, 1)
    api.add_array_field("stars_array", arrays[0][2], 0)
    a = api.slice(flat.path, 40, 30, "stars", axis="z")
    b = api.slice(flat.path, 40, 30, "stars_array", axis="z")
    assert same(a, b) and np.isfinite(a).any()
    a = api.profile(flat.path, "stars", "u", bins=8)
    b = api.profile(flat.path, "stars_array", "u", bins=8)
    assert same(a["x_edges"], b["x_edges"])
    assert np.array_equal(a["cells"], b["cells"]) and int(a["cells"].sum()) == 16 * 8 * 8


def test_particle_cells_gives_levels_ordinals_and_centres(ctx, patched):
    points = np.concatenate([special_positions(patched), random_particles(patched, 500, 93)[0]])
    h = patched.hierarchy()
    level, _, index = h.locate(points)
    got = api.particle_cells(patched.path, points)
    assert np.array_equal(got["level"], np.where(level < 0, 255, level).astype(np.uint8))
    found = pr.contributions(h, points, None, 0)
    want = expected_cells(patched, found)[:, 0]
    assert np.array_equal(got["ordinal"], np.where(level < 0, -1, want))
    centres = np.full((len(points), 3), np.nan)
    for l in range(2):
        pick = level == l
        centres[pick] = np.array(patched.lo) + (index[pick].astype(np.float64) + 0.5) * \
            np.array(patched.sizes()[l])
    assert same(got["centres"], centres) and (level < 0).any() and (level == 1).any()
    # on the coarse level alone every particle inside has level 0
    got = api.particle_cells(patched.path, points, max_level=0)
    assert set(got["level"].tolist()) == {0, 255}


def test_products_of_stored_variables_are_unchanged_around_a_particle_field(ctx, patched):
    before = api.slice(patched.path, 40, 30, "u", axis="y")
    api.add_particle_field("stars", *dyadic_particles(patched, 200, 95))
    assert np.isfinite(api.slice(patched.path, 40, 30, "stars", axis="y")).any()
    after = api.slice(patched.path, 40, 30, "u", axis="y")
    assert same(before, after)
