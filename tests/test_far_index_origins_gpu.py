"""The products that cross levels on hierarchies whose index ranges end on the limits of the index
rule (box_index_region in avr_field_plans.h): the level-0 domain, refined to the finest level, ends
at index 2^30 - 1 or begins at -2^30 (wide_view_cases.far_hierarchies and translations, held to
their claims by test_wide_view_cases.py).  The scenes are made at the runtime level, from the
hierarchy's leaf boxes and the translated box_index_lo.

Products that work in index space alone give the bits of the untranslated run, and every index
they report is shifted by exactly the translation.  Products in physical coordinates get
prob_lo' = prob_lo - T_0 * size_0 with power-of-two cell sizes, so that the physical domain is
unchanged and every cell face exactly representable, and are compared with the product's own
float64 reference run on the translated levels, by the comparator of the product's own GPU test:
bit for bit.

Covered: gradient, clumps with their table and links, covering grids, derive, isosurfaces,
streamlines, rays and ray sums; and, of the products merged since, grid fields (index space alone),
particle cells and deposits (floor_div and box_holds on negative indices, cloud corners one cell
past either limit), ray transfer (grey and sharp by bits, broadened within the reference's own
a-priori bounds) and clump members with their data (the centres from prob_lo' + (index + 1/2) dx).
Left out: structure functions, the FFT products and particle groups take contiguous tensors and no
box indices, and velocity cubes take physical coordinates only, so the index rule does not apply
to them."""
import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import api, plotfile
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform

import binding_reference
import clump_reference
import isosurface_reference
import particle_reference as pr
import ray_reference
import ray_sums_reference
import ray_transfer_reference
import streamline_reference
import wide_view_cases as cases
from gradient_reference import VARIABLES, same_bits
from test_ray_transfer_gpu import same_transfer
from test_wide_view_cases import far_conditions

pytestmark = pytest.mark.gpu
HIERARCHIES = cases.far_hierarchies()
PLACES = [(h, where) for h in HIERARCHIES for where in ("top", "bottom")]
IDS = [f"{h.name}-{where}" for h, where in PLACES]
SIZE_0 = cases.FAR_SIZE_0            # a power of two; the finer levels divide it by their ratios
PROB_LO = cases.FAR_PROB_LO
U, ODD, WHOLE = (VARIABLES.index(name) for name in ("u", "odd", "whole"))


class Placed:
    """A hierarchy at a translation (None: where far_hierarchies puts it): its leaf boxes as
    contiguous device tensors, their indices, the cell sizes and prob_lo'."""

    def __init__(self, ctx, h, translation):
        self.ctx, self.h = ctx, h
        self.levels = cases.far_levels(h, translation)
        self.shift = translation if translation is not None else [(0, 0, 0)] * 3
        refine = [1, h.ratio[0], h.ratio[0] * h.ratio[1]]
        self.sizes = [(SIZE_0 / r,) * 3 for r in refine]
        self.prob_lo = tuple(PROB_LO[a] - self.shift[0][a] * SIZE_0 for a in range(3))
        convex = plotfile.convexify([lev["boxes"] for lev in self.levels], h.ratio)
        self.scene_boxes, self.grids = [], []
        for level, entries in enumerate(convex):
            for grid, (lo, hi) in entries:
                self.scene_boxes.append((level, lo, hi))
                self.grids.append(grid)
        self.index_lo = np.array([lo for _, lo, _ in self.scene_boxes], dtype=np.int32)

    def corners(self, box):
        level, lo, hi = self.scene_boxes[box]
        size = self.sizes[level][0]
        return (tuple(self.prob_lo[a] + lo[a] * size for a in range(3)),
                tuple(self.prob_lo[a] + (hi[a] + 1) * size for a in range(3)))

    def boxes(self, component=None):
        """The leaf boxes with one field's cells (a stored component, or what a function makes
        of a grid's stored components), or with cells to write into."""
        out = []
        for box, ((level, lo, hi), grid) in enumerate(zip(self.scene_boxes, self.grids)):
            glo = self.levels[level]["boxes"][grid][0]
            cut = tuple(slice(lo[a] - glo[a], hi[a] - glo[a] + 1) for a in (2, 1, 0))
            if component is None:
                shape = tuple(s.stop - s.start for s in cut)
                values = torch.full(shape, 1e300, dtype=torch.float64, device=self.ctx.device)
            else:
                data = self.levels[level]["data"][grid]
                cells = np.ascontiguousarray((component(data) if callable(component)
                                              else data[component])[cut])
                values = torch.from_numpy(cells).to(self.ctx.device)
            out.append(AmrBox(*self.corners(box), values, level))
        return out

    def scene(self, component=None):
        return self.ctx.create_scene(self.boxes(component), ScalarTransform())

    def level_arguments(self):
        return self.index_lo, self.h.ratio, self.sizes, self.prob_lo

    def points(self, n, seed):
        """n points of the physical domain, a tenth of it beyond each side included; the domain is
        where PROB_LO puts it, whatever the translation."""
        return cases.far_points(self.h, n, seed)


@pytest.fixture(scope="module", params=PLACES, ids=IDS)
def pair(request, ctx):
    h, where = request.param
    return Placed(ctx, h, cases.translations(h)[where]), Placed(ctx, h, None)


def test_the_scene_is_the_untranslated_one_moved_by_the_translation(pair):
    far, near = pair
    assert len(far.scene_boxes) == len(near.scene_boxes) > 3 and far.grids == near.grids
    assert {level for level, _, _ in far.scene_boxes} == {0, 1, 2}
    for box, ((level, lo, hi), (was_level, was_lo, was_hi)) in enumerate(zip(far.scene_boxes,
                                                                            near.scene_boxes)):
        t = far.shift[level]
        assert level == was_level
        assert lo == tuple(was_lo[a] + t[a] for a in range(3))
        assert hi == tuple(was_hi[a] + t[a] for a in range(3))
        assert far.corners(box) == near.corners(box)         # exactly: the physical domain stays
    finest = far.index_lo[[level == 2 for level, _, _ in far.scene_boxes]]
    assert np.abs(finest.astype(np.int64)).max() > 2 ** 30 - 64
    assert all(np.frexp(s[0])[0] == 0.5 for s in far.sizes)                 # powers of two
    assert all(float(v) == int(v * 16) / 16 for v in far.prob_lo)


# ---- products in index space ----------------------------------------------------------------------

def _written(ctx, placed, run):
    out = placed.scene()
    extra = run(out)
    ctx.synchronize()
    return [b.values.cpu().numpy() for b in out.boxes], extra


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_gradient_gives_the_bits_of_the_untranslated_run(ctx, pair, axis):
    for component in (U, ODD):
        results = []
        for placed in pair:
            sizes = [s[axis] for s in placed.sizes]
            results.append(_written(ctx, placed, lambda out: out.gradient(
                placed.scene(component), axis, placed.index_lo, placed.h.ratio, sizes))[0])
        for got, want in zip(*results):
            assert same_bits(got, want)
            assert (got != 1e300).all()


def test_clumps_their_table_and_their_links(ctx, pair):
    results = []
    for placed in pair:
        def run(out):
            count = out.clumps(placed.scene(U), -0.25, 10.0, placed.index_lo, placed.h.ratio)
            ctx.synchronize()
            n = int(count.item())
            table = out.clump_table(n, 3, placed.scene(WHOLE))      # integers: exact sums
            links = out.clump_links(n, placed.index_lo, placed.h.ratio)
            ctx.synchronize()
            return n, [t.cpu().numpy() for t in table], links[0].cpu().numpy(), links[3].cpu().numpy()
        results.append(_written(ctx, placed, run))
    (labels, (n, table, extent, totals)), (was_labels, (was_n, was_table, was_extent, was_totals)) = \
        results
    assert n == was_n >= 1
    for got, want in zip(labels, was_labels):
        assert same_bits(got, want)
    for got, want in zip(table, was_table):
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert np.array_equal(totals, was_totals)
    # the bounding boxes are in the finest level's index space: moved by T_2, lows and highs alike
    t = np.array(pair[0].shift[2] * 2, dtype=np.int64)
    assert extent.dtype == np.int32 and extent.shape == (6, n)
    assert np.array_equal(extent.astype(np.int64), was_extent.astype(np.int64) + t[:, None])
    assert (was_extent[:3] <= was_extent[3:]).all()


@pytest.mark.parametrize("level", [0, 1, 2])
def test_covering_grid_of_a_whole_level(ctx, pair, level):
    results = []
    for placed in pair:
        lo, hi = placed.levels[level]["domain"]
        dims = tuple(hi[a] - lo[a] + 1 for a in range(3))
        grid = placed.scene(ODD).covering_grid(level, lo, dims, placed.index_lo, placed.h.ratio)
        ctx.synchronize()
        results.append([t.cpu().numpy() for t in grid])
    for got, want in zip(*results):
        assert got.dtype == want.dtype and got.shape == want.shape
        assert same_bits(got, want) if got.dtype == np.float64 else np.array_equal(got, want)
    assert results[0][1].min() == 1.0 and results[0][2].max() == 2       # covered; finest leaves


# ---- products in physical coordinates ----------------------------------------------------------

def test_derive_sees_the_same_box_origins(ctx, pair):
    """derive takes no index: the grid built-ins come from box_origin, which is prob_lo' + index *
    size on the host, exactly the untranslated origin."""
    program = api.compile_expression("field('a') + x * 2.0 + y - z * level + dx * cell_volume")
    results = []
    for placed in pair:
        origin = [placed.corners(b)[0] for b in range(len(placed.scene_boxes))]
        results.append((origin, _written(ctx, placed, lambda out: out.derive(
            [placed.scene(U)], program.instructions, program.constants, origin, placed.sizes))[0]))
    assert results[0][0] == results[1][0]
    for got, want in zip(results[0][1], results[1][1]):
        assert same_bits(got, want) and (got != 1e300).all()


def test_isosurface_is_the_reference_on_the_translated_levels(ctx, pair):
    far = pair[0]
    counts = far.scene(U).isosurface(0.25, *far.level_arguments(), far.scene(WHOLE))[0]
    ctx.synchronize()
    triangles, skipped = (int(v) for v in counts.cpu().numpy())
    counts, vertices, levels, samples = far.scene(U).isosurface(
        0.25, *far.level_arguments(), far.scene(WHOLE), capacity=triangles)
    ctx.synchronize()
    want = isosurface_reference.isosurface(far.levels, far.h.ratio, U, 0.25, far.scene_boxes,
                                           far.sizes, far.prob_lo, sample_component=WHOLE)
    assert triangles == want["vertices"].shape[0] > 100 and skipped == want["skipped"]
    assert same_bits(vertices.cpu().numpy(), want["vertices"])
    assert levels.dtype == torch.uint8 and np.array_equal(levels.cpu().numpy(), want["level"])
    assert same_bits(samples.cpu().numpy(), want["samples"])
    assert {1, 2} <= set(want["level"].tolist())


@pytest.mark.parametrize("direction", [1, -1])
def test_streamlines_are_the_reference_on_the_translated_levels(ctx, pair, direction):
    far = pair[0]
    seeds, max_steps = far.points(48, 1), 24
    vx, vy, vz, sample = (far.scene(c) for c in (U, WHOLE, ODD, U))
    points, samples, counts, status = vx.streamlines(vy, vz, seeds, 0.5, direction, max_steps,
                                                     *far.level_arguments(), sample)
    ctx.synchronize()
    want = streamline_reference.trace(far.levels, far.h.ratio, (U, WHOLE, ODD), far.sizes,
                                      far.prob_lo, seeds, 0.5, direction, max_steps, sample=U)
    assert np.array_equal(status.cpu().numpy(), want["status"])
    assert np.array_equal(counts.cpu().numpy(), want["counts"])
    assert same_bits(points.cpu().numpy(), want["points"])
    assert same_bits(samples.cpu().numpy(), want["samples"])
    assert (want["counts"] > 3).sum() > 10


def _ray_ends(far):
    start, end = far.points(96, 2), far.points(96, 3)
    lo, hi = far.h.domains[0]
    high = np.array([PROB_LO[a] + (hi[a] - lo[a] + 1) * SIZE_0 for a in range(3)])
    start[0], end[0] = np.array(PROB_LO), high                               # the diagonal
    start[1], end[1] = high + 0.125, np.array(PROB_LO) - 0.125
    start[2], end[2] = (PROB_LO[0] - 0.5, PROB_LO[1] + 0.5, PROB_LO[2] + 0.5), \
        (high[0] + 0.5, PROB_LO[1] + 0.5, PROB_LO[2] + 0.5)                  # in cell faces
    return start, end


def test_rays_are_the_reference_on_the_translated_levels(ctx, pair):
    far = pair[0]
    start, end = _ray_ends(far)
    hierarchy = ray_reference.Hierarchy(far.levels, far.h.ratio, ODD, far.sizes, far.prob_lo, 0, -1)
    max_trips = hierarchy.default_max_trips()
    want = hierarchy.rays(start, end, max_trips)
    scene = far.scene(ODD)
    counts, status, span = scene.rays(start, end, max_trips, *far.level_arguments())
    ctx.synchronize()
    offsets = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=ctx.device)
    offsets[1:] = torch.cumsum(counts.to(torch.int64), 0)
    assert np.array_equal(offsets.cpu().numpy(), want["offsets"])
    assert np.array_equal(status.cpu().numpy(), want["status"])
    assert same_bits(span.cpu().numpy()[:, 0], want["t_enter"])
    assert same_bits(span.cpu().numpy()[:, 1], want["t_leave"])
    t0, t1, level, value, integral, covered = scene.rays(
        start, end, max_trips, *far.level_arguments(), offsets=offsets,
        n_segments=int(want["offsets"][-1]))
    ctx.synchronize()
    assert level.dtype == torch.int8 and np.array_equal(level.cpu().numpy(), want["level"])
    for got, key in ((t0, "t0"), (t1, "t1"), (value, "value"), (integral, "integral"),
                     (covered, "covered")):
        assert same_bits(got.cpu().numpy(), want[key]), key
    assert set(want["level"].tolist()) >= {0, 1, 2} and (want["status"] == 0).sum() > 40


@pytest.mark.parametrize("weighted", [False, True])
def test_ray_sums_are_the_reference_on_the_translated_levels(ctx, pair, weighted):
    far = pair[0]
    start, end = _ray_ends(far)
    field = ray_reference.Hierarchy(far.levels, far.h.ratio, ODD, far.sizes, far.prob_lo, 0, -1)
    weight = ray_reference.Hierarchy(far.levels, far.h.ratio, WHOLE, far.sizes, far.prob_lo, 0, -1)
    want = ray_sums_reference.ray_sums(start, end, field, weight if weighted else None)
    counts, status, span, integral, weight_sum, counted, covered = far.scene(ODD).ray_sums(
        start, end, field.default_max_trips(), *far.level_arguments(),
        weight=far.scene(WHOLE) if weighted else None)
    ctx.synchronize()
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), want["count"])
    assert np.array_equal(status.cpu().numpy(), want["status"])
    assert same_bits(span.cpu().numpy()[:, 0], want["t_enter"])
    assert same_bits(span.cpu().numpy()[:, 1], want["t_leave"])
    for got, key in ((integral, "integral"), (counted, "counted"), (covered, "covered")):
        assert same_bits(got.cpu().numpy(), want[key]), key
    assert (weight_sum is None) == (not weighted)
    if weighted:
        assert same_bits(weight_sum.cpu().numpy(), want["weight"])


# ---- the products merged after this module was written -----------------------------------------

GRID_MODES = [(0, False), (1, False), (1, True)]        # (interpolation, periodic)


@pytest.mark.parametrize("level", [0, 1, 2])
def test_grid_field_gives_the_bits_of_the_untranslated_run(ctx, pair, level):
    """Index space alone: a grid over the level's whole domain, its lo moved by T_level, and at
    level 1 another over half of it and one column more, which cuts coarse cells.  With ratios 2
    and 4 every interpolation weight is dyadic."""
    results = []
    for placed in pair:
        lo, hi = placed.levels[level]["domain"]
        dims = tuple(hi[a] - lo[a] + 1 for a in range(3))
        grids = [cases.far_grid(dims, level)]
        if level == 1:
            grids.append(cases.far_grid((dims[0] // 2 + 1, dims[1], dims[2]), 9))
        runs = []
        for grid in grids:
            device_grid = torch.from_numpy(grid).to(ctx.device)
            for interpolation, periodic in GRID_MODES:
                cells, totals = _written(ctx, placed, lambda out: out.grid_field(
                    device_grid, level, lo, placed.index_lo, placed.h.ratio, interpolation,
                    periodic))
                runs.append((cells, totals.tolist()))
        results.append(runs)
    assert len(results[0]) == len(results[1]) == (6 if level == 1 else 3)
    for n, ((got, totals), (want, was_totals)) in enumerate(zip(*results)):
        assert totals == was_totals
        assert totals == [0, 0] if n < 3 else (totals[0] > 0 and totals[1] > 0)
        for a, b in zip(got, want):
            assert same_bits(a, b) and (a != 1e300).all()


def _ordinal_maps(placed):
    """Per level the cell ordinal over the level's domain, -1 where no scene box holds the cell:
    the cells of the boxes in scene order, (k ny + j) nx + i inside a box."""
    maps = []
    for lev in placed.levels:
        lo, hi = lev["domain"]
        maps.append(np.full(tuple(hi[a] - lo[a] + 1 for a in (2, 1, 0)), -1, dtype=np.int64))
    begin = 0
    for level, lo, hi in placed.scene_boxes:
        view = _cut(placed, maps, level, lo, hi)
        view[...] = begin + np.arange(view.size).reshape(view.shape)
        begin += view.size
    return maps


def _cut(placed, dense, level, lo, hi):
    dlo = placed.levels[level]["domain"][0]
    return dense[level][lo[2] - dlo[2]:hi[2] - dlo[2] + 1, lo[1] - dlo[1]:hi[1] - dlo[1] + 1,
                        lo[0] - dlo[0]:hi[0] - dlo[0] + 1]


@pytest.mark.parametrize("method", [0, 1])
def test_particles_are_the_reference_on_the_translated_levels(ctx, pair, method):
    """floor_div and box_holds on indices next to -2^30 and 2^30, and cloud corners one cell past
    them: cells, shares, levels and the deposited boxes by bits, the totals equal, as
    test_particles_gpu.check_cells compares them."""
    far = pair[0]
    p = cases.far_particles(far.h)
    h = pr.hierarchy(far.levels, far.h.ratio, far.sizes, far.prob_lo)
    found = pr.contributions(h, p.points, p.values, method)
    clouds = found if method == 1 else pr.contributions(h, p.points, p.values, 1)
    leaves = far_conditions(far.h, "top" if far.shift[0][0] > 0 else "bottom", h, clouds, p.points)
    print("leaves per level", leaves.tolist(), "outside", found["outside"], "rerouted",
          found["rerouted"])
    runs = []
    for placed in pair:
        out = placed.scene()
        cells, shares, levels, totals = out.particle_cells(
            p.points, p.values, method, *placed.level_arguments(), levels=True)
        ctx.synchronize()
        boxes = []
        for quantity in (0, 1):
            out.particle_deposit(cells, shares, quantity, placed.sizes)
            ctx.synchronize()
            boxes.append([b.values.cpu().numpy() for b in out.boxes])
        runs.append((cells.cpu().numpy(), shares.cpu().numpy(), levels.cpu().numpy(),
                     totals.tolist(), boxes))
    cells, shares, levels, totals, boxes = runs[0]
    assert totals == [found["outside"], found["rerouted"]]
    maps = _ordinal_maps(far)
    expected = np.full(found["level"].shape, 0xFFFFFFFF, dtype=np.int64)
    for l, lev in enumerate(far.levels):
        pick = found["level"] == l
        rel = found["index"][pick] - np.array(lev["domain"][0])[None, :]
        expected[pick] = maps[l][rel[:, 2], rel[:, 1], rel[:, 0]]
    assert (expected >= 0).all() and np.array_equal(cells, expected)
    assert same_bits(shares, found["shares"])
    assert np.array_equal(levels, np.where(found["leaf_level"] < 0, 255, found["leaf_level"]))
    for quantity in (0, 1):
        dense = pr.deposit(h, found, quantity)
        for got, (level, lo, hi) in zip(boxes[quantity], far.scene_boxes):
            want = _cut(far, dense, level, lo, hi)
            assert same_bits(got, want), (level, lo, hi)
            numbers = ~np.isnan(want)           # +0.0 by its bits where nothing lands
            assert np.array_equal(got.view(np.uint64)[numbers], want.view(np.uint64)[numbers])
    # the lattice batch is exact under the translation: the untranslated run's cells and shares
    was_cells, was_shares, _, was_totals, _ = runs[1]
    assert np.array_equal(cells[p.lattice], was_cells[p.lattice])
    assert same_bits(shares[p.lattice], was_shares[p.lattice])
    assert totals == was_totals


_WALKS = {}


def _walked(far, start, end):
    """ray_reference's walk of the four transfer fields on the translated levels, made once per
    place: ({name: walk}, max_trips)."""
    key = (far.h.name, far.shift[0])
    if key not in _WALKS:
        walks, max_trips = {}, None
        for name in cases.FAR_FIELDS:
            hierarchy = ray_reference.Hierarchy(cases.far_field_levels(far.levels, name),
                                                far.h.ratio, 0, far.sizes, far.prob_lo, 0, -1)
            max_trips = hierarchy.default_max_trips()
            walks[name] = hierarchy.rays(start, end, max_trips)
        _WALKS[key] = (walks, max_trips)
    return _WALKS[key]


TRANSFERS = {"grey": (("source", "opacity", None, None), None),
             "sharp": (("source", "opacity", "bin", None), cases.FAR_SHARP_EDGES),
             "broadened": (("source", "opacity", "bin", "width"), cases.FAR_BROAD_EDGES)}


@pytest.mark.parametrize("mode", list(TRANSFERS))
def test_ray_transfer_is_the_reference_on_the_translated_levels(ctx, pair, mode):
    """The fields are mapped from the stored components once, in numpy, for the device boxes and
    for the reference's levels alike; the comparator is test_ray_transfer_gpu's."""
    far = pair[0]
    start, end = _ray_ends(far)
    walks, max_trips = _walked(far, start, end)
    names, edges = TRANSFERS[mode]
    want = ray_transfer_reference.transfer_of(
        start, end, *(walks[name] if name else None for name in names), edges=edges)
    scenes = [far.scene(cases.FAR_FIELDS[name]) if name else None for name in names]
    counts, status, span, intensity, tau, outside, counted, covered = scenes[0].ray_transfer(
        scenes[1], start, end, max_trips, *far.level_arguments(), scenes[2], scenes[3], edges)
    ctx.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    got = {"count": host(counts).view(np.uint32), "status": host(status),
           "t_enter": host(span)[:, 0].copy(), "t_leave": host(span)[:, 1].copy(),
           "intensity": host(intensity), "tau": host(tau), "outside": host(outside),
           "counted": host(counted), "covered": host(covered)}
    same_transfer(got, want, mode == "broadened")
    assert (want["status"] == 0).sum() > 40
    assert set(walks["source"]["level"].tolist()) >= {0, 1, 2}
    assert (want["tau"] > 0.0).any(axis=1).all()
    if edges is not None:
        assert (want["outside"] > 0.0).any(axis=1).all()


def test_clump_members_and_their_data(ctx, pair):
    """Keys (ordinals are per scene) and the values of the field of integers equal the untranslated
    run's; levels and centres equal binding_reference.members on the translated levels and, the
    physical domain being unchanged and everything dyadic, the untranslated run's by bits."""
    results = []
    for placed in pair:
        def run(out):
            count = out.clumps(placed.scene(U), -0.25, 10.0, placed.index_lo, placed.h.ratio)
            ctx.synchronize()
            n = int(count.item())
            cells = out.clump_table(n, 3)[0]
            ctx.synchronize()
            keys, totals = out.clump_members(n, np.ones(n, dtype=np.uint8), int(cells.sum().item()))
            levels, centres, values = out.clump_member_data(
                keys, *placed.level_arguments(), field=placed.scene(WHOLE))
            ctx.synchronize()
            return n, totals.tolist(), keys.cpu().numpy(), levels.cpu().numpy(), \
                centres.cpu().numpy(), values.cpu().numpy()
        results.append(_written(ctx, placed, run)[1])
    (n, totals, keys, levels, centres, values), (was_n, _, was_keys, was_levels, was_centres,
                                                 was_values) = results
    assert n == was_n >= 1 and totals == [0] and keys.size > 100
    assert np.array_equal(keys, was_keys) and same_bits(values, was_values)
    assert np.array_equal(levels, was_levels) and same_bits(centres, was_centres)
    far = pair[0]
    labels, want_n = clump_reference.clump_levels(far.levels, far.h.ratio, U, -0.25, 10.0,
                                                  far.scene_boxes)
    want = binding_reference.members(labels, want_n, [1] * want_n, far.levels, far.h.ratio,
                                     far.scene_boxes, far.prob_lo, far.sizes, (WHOLE,))
    assert n == want_n and keys.tolist() == want["keys"]
    assert levels.dtype == np.uint8 and np.array_equal(levels, want["level"])
    assert same_bits(centres.T, want["centres"]) and same_bits(values, want["values"][WHOLE])
    assert set(want["level"].tolist()) == {0, 1, 2}
