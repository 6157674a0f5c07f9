"""Every cell-reading entry point on boxes at the span limit of field_view (avr_field_boxes.h): views
that span up to 2^28 - 1 elements of a 2 GiB storage, so that byte offsets use bit 30 and end at
2^31 - 8 (tests/wide_view_cases.py, held to its claims by tests/test_wide_view_cases.py).

The contiguous path of each product is held to the oracle and the numpy references by the
product's own tests.  The claim here is that a result does not depend on the layout: each call is
made twice, on the views and on contiguous copies of the same cells with the same corners, levels
and indices, and the results must be equal bit for bit, NaN equal to NaN.  The storage around the
views holds one poison bit pattern; after a product that writes cells the output view's cells are
copied out, poison is written back over them, and one device reduction checks that the whole
output storage is poison again and the input storage unchanged.

Covered: the painter and the frames, the statistics and histograms, slices, axis projections,
derive, gradient, clumps with their table and links, covering grids, isosurfaces, streamlines, rays
and ray sums; and, of the products merged since, velocity cubes, ray transfer, grid fields,
particle cells and deposits, and clump members with their data.  For those the numpy references
also say what the wide box's last cells must hold, mixed runs (some fields views, some copies)
hold the AND over the fields' pairing flags, and one sensitivity test per product shows that the
wide box's last cell reaches the result.  Left out: structure functions, the FFT products and
particle groups take contiguous tensors and no boxes, so the span rule does not apply to them."""
import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import api, scenes
from amrvolumerenderer_amd.renderer import FrameRenderer, RenderParameters
from amrvolumerenderer_amd.types import (AmrBox, CameraParameters, ScalarTransform, VolumeBounds,
                                         make_params)

import grid_field_reference
import particle_reference
import wide_view_cases as cases
from gradient_reference import same_bits
from test_wide_view_cases import wide_hierarchy

pytestmark = pytest.mark.gpu
CASES = cases.wide_cases()
W, H = 48, 32
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
BOUNDS = VolumeBounds((-0.05,) * 3, (1.05,) * 3)
# field 0 lies in (1, 2): its own range as the unit range
NORM = ScalarTransform(normalize_to_unit_range=True, normalization_min=1.0, normalization_max=2.0,
                       inverse_normalization_span=1.0)
CAMERAS = [scenes.default_camera(),
           CameraParameters((1.7, -0.6, 2.1), (0.45, 0.55, 0.5), (0.1, 1.0, 0.2), 40.0, 0.1, 20.0)]
SIZES = cases.level_sizes()
ORIGIN = (0.0, 0.0, 0.0)


def strided(storage, view):
    nx, ny, nz = view.dims
    return torch.as_strided(storage, (nz, ny, nx), (view.kstride, view.jstride, 1), view.offset)


def not_poison(storage):
    """How many elements of a storage differ from the poison by bits: one device reduction."""
    return int((storage.view(torch.int64) != cases.POISON_BITS).sum().item())


def bits(t):
    return t.contiguous().view(torch.int64)


def assert_same(got, want, what):
    """Tensors equal by bits (NaN equal to NaN), tuples and lists member by member."""
    if isinstance(want, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(want), what
        for n, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, (what, n))
    elif isinstance(want, torch.Tensor):
        assert got.dtype == want.dtype and got.shape == want.shape, what
        if want.dtype == torch.float64:
            assert same_bits(got.cpu().numpy(), want.cpu().numpy()), what
        else:
            assert torch.equal(got, want), what
    else:
        assert got == want, (what, got, want)


@pytest.fixture(scope="module")
def storages(ctx):
    """The input and the output storage, poison everywhere, made on the device."""
    torch.cuda.synchronize(ctx.device)
    torch.cuda.reset_peak_memory_stats(ctx.device)
    pair = [torch.full((cases.STORAGE,), cases.POISON, dtype=torch.float64, device=ctx.device)
            for _ in range(2)]
    for t in pair:
        assert t.data_ptr() % 16 == 0
    assert not_poison(pair[0]) == 0 and not_poison(pair[1]) == 0
    yield pair
    ctx.synchronize()
    print("peak device memory of this module: %.2f GiB"
          % (torch.cuda.max_memory_allocated(ctx.device) / 2.0 ** 30))


class Installed:
    """A case's six fields written through their views into the input storage, contiguous copies
    of them, the ordinary boxes of the case's scene, and the output view in the second storage."""

    def __init__(self, ctx, case, inputs, outputs):
        self.ctx, self.case, self.inputs, self.outputs = ctx, case, inputs, outputs
        device = ctx.device
        self.host = [cases.field_cells(case, f, odd=(f == 0)) for f in range(cases.MAX_FIELDS)]
        self.views, self.dense = [], []
        for f, cells in enumerate(self.host):
            view = cases.field_view(case, f)
            t = strided(inputs, view)
            t.copy_(torch.from_numpy(cells).to(device))
            assert t.data_ptr() % 16 == 8 * (view.offset % 2)
            assert (t.stride(0), t.stride(1)) == (view.kstride, view.jstride)
            self.views.append(t)
            self.dense.append(t.contiguous())
            assert self.dense[f].data_ptr() % 16 == 0 and self.dense[f].is_contiguous()
        self.n_cells = sum(c.size for c in self.host)
        by_kind = {b.kind: b for b in cases.hierarchy(case)}
        self.small = {kind: [torch.from_numpy(cases.small_cells(by_kind[kind].dims, tag + f)).to(device)
                             for f in range(cases.MAX_FIELDS)]
                      for kind, tag in (("plain", 0), ("fine", 10))}
        self.out_view = strided(outputs, case.view)
        self.check_storages()

    def remove(self):
        for t in self.views:
            t.fill_(cases.POISON)
        assert not_poison(self.inputs) == 0 and not_poison(self.outputs) == 0

    def check_storages(self):
        """The output storage is poison everywhere; the input storage holds the fields and poison."""
        assert not_poison(self.outputs) == 0
        assert not_poison(self.inputs) == self.n_cells
        for view, copy in zip(self.views, self.dense):
            assert torch.equal(bits(view), bits(copy))

    def boxes(self, field, wide, wide_first=True):
        """The case's scene for one field: the wide box as a view or as its contiguous copy."""
        out = []
        for b in cases.hierarchy(self.case, wide_first):
            values = ((self.views if wide else self.dense)[field] if b.kind == "wide"
                      else self.small[b.kind][field])
            out.append(AmrBox(*cases.corners(b), values, b.level))
        return out

    def scene(self, field, wide, wide_first=True):
        return self.ctx.create_scene(self.boxes(field, wide, wide_first), ScalarTransform())

    def changed_scene(self, field, at, value):
        """The contiguous layout with cell `at` of the wide box replaced by value."""
        boxes = self.boxes(field, False)
        cells = boxes[0].values.clone()
        assert float(cells[at].item()) != value
        cells[at] = value
        boxes[0] = AmrBox(boxes[0].min_corner, boxes[0].max_corner, cells, boxes[0].level)
        return self.ctx.create_scene(boxes, ScalarTransform())

    def scaled(self, field, factor):
        return _Scaled(self, field, factor)

    def index_lo(self, wide_first=True):
        return np.array([b.index_lo for b in cases.hierarchy(self.case, wide_first)], dtype=np.int32)

    def output_scene(self, wide, wide_first=True):
        """A scene to write into: the wide box is the view in the output storage, or a contiguous
        tensor; the ordinary boxes are contiguous tensors.  Everything starts as poison."""
        out = []
        for b in cases.hierarchy(self.case, wide_first):
            nx, ny, nz = b.dims
            values = self.out_view if (wide and b.kind == "wide") else torch.full(
                (nz, ny, nx), cases.POISON, dtype=torch.float64, device=self.ctx.device)
            out.append(AmrBox(*cases.corners(b), values, b.level))
        return self.ctx.create_scene(out, ScalarTransform()), [b.values for b in out]

    def written(self, run):
        """run(wide, wide_first, output scene) on the views and on the copies, in both box orders:
        the cells written (and whatever run returns) are equal, nothing but the output view's
        cells was written in the output storage, and the input storage is unchanged."""
        for wide_first in (True, False):
            results = []
            for wide in (True, False):
                scene, tensors = self.output_scene(wide, wide_first)
                extra = run(wide, wide_first, scene)
                self.ctx.synchronize()
                results.append(([t.clone() for t in tensors], extra))
                if wide:
                    self.out_view.fill_(cases.POISON)
                    self.check_storages()
            assert_same(results[0], results[1], (self.case.name, wide_first))
            for cells in results[1][0]:
                assert not_poison(cells) == cells.numel()       # every cell was written
        return results[1]

    def read(self, run):
        """run(wide, wide_first) on the views and on the copies, in both box orders."""
        for wide_first in (True, False):
            got = run(True, wide_first)
            self.ctx.synchronize()
            want = run(False, wide_first)
            self.ctx.synchronize()
            assert_same(got, want, (self.case.name, wide_first))
        return want


@pytest.fixture(scope="module", params=CASES, ids=[c.name for c in CASES])
def wide(request, ctx, storages):
    installed = Installed(ctx, request.param, *storages)
    yield installed
    ctx.synchronize()
    installed.remove()


def test_views_are_what_the_case_says(wide):
    case = wide.case
    for f, t in enumerate(wide.views):
        paired = t.data_ptr() % 16 == 0 and t.stride(0) % 2 == 0 and t.stride(1) % 2 == 0
        assert paired == case.others_pair
        assert (paired and t.stride(1) < 2 ** 27) == case.classify_pairs
        last = t.stride(0) * (t.shape[0] - 1) + t.stride(1) * (t.shape[1] - 1) + t.shape[2] - 1
        assert last == cases.span(case.view) and 8 * last >= 2 ** 30
        assert same_bits(t.cpu().numpy(), wide.host[f])


# ---- the painter and the frames ---------------------------------------------------------------

def _paint(ctx, call, values, cam, with_transform=True):
    samples = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    box = AmrBox(*UNIT, values)
    params = make_params(W, H, (0.0, 1.0), 0.0, 0.0, BOUNDS)
    arguments = (box, NORM, params, cam) if with_transform else (box, params, cam)
    out = call(*arguments, samples=samples)
    ctx.synchronize()
    out = tuple(t.clone() for t in out) if isinstance(out, tuple) else out.clone()
    return out, int(samples.item())


@pytest.mark.parametrize("view", [0, 1])
def test_paint_box_and_paint_box_max(ctx, wide, view):
    """classify_tile on the view, then the march of its bricklets.  For the end pair this is the
    16-byte buffer load at offset 2^31 - 16 of a resource of 2^31 - 1 records."""
    cam = CAMERAS[view]
    for f in (0, 1):    # with NaN / +-Inf cells, and without
        transform = NORM if f == 0 else ScalarTransform(
            normalize_to_unit_range=True, normalization_min=2.0, normalization_max=3.0,
            inverse_normalization_span=1.0)
        for call in (ctx.paint_box, ctx.paint_box_max):
            def run(values):
                samples = torch.zeros(1, dtype=torch.int64, device=ctx.device)
                out = call(AmrBox(*UNIT, values), transform,
                           make_params(W, H, (0.0, 1.0), 0.0, 0.0, BOUNDS), cam, samples=samples)
                ctx.synchronize()
                return out.clone(), int(samples.item())
            got, want = run(wide.views[f]), run(wide.dense[f])
            assert want[1] > 0
            assert_same(got, want, (wide.case.name, f, call.__name__))
        # the box's last cell holds the field's maximum and faces the default camera: the largest
        # table index of the frame is that cell's, where the cells are large enough to be sampled
        if view == 0 and wide.case.view.dims[0] <= 7:
            last = np.float32(wide.host[f][-1, -1, -1] - (1.0 + f))
            assert int(got[0].max().item()) == int(np.float32(last * np.float32(255.0)))


@pytest.mark.parametrize("view", [0, 1])
def test_paint_box_projection(ctx, wide, view):
    """The projection march addresses the raw cells by 32-bit byte offsets up to 2^31 - 8."""
    for f in (0, 1):
        got = _paint(ctx, ctx.paint_box_projection, wide.views[f], CAMERAS[view], False)
        want = _paint(ctx, ctx.paint_box_projection, wide.dense[f], CAMERAS[view], False)
        assert want[1] > 0 and float(want[0][0].max().item()) > 0.0
        assert_same(got, want, (wide.case.name, f))


def test_render_and_render_projection_frames(ctx, wide):
    """One volume frame and one projection frame of the three boxes side by side in the unit cube."""
    edges = [0.0, 0.4, 0.7, 1.0]
    frames = []
    for layout in (True, False):
        values = [(wide.views if layout else wide.dense)[0], wide.small["plain"][0],
                  wide.small["fine"][0]]
        local = [AmrBox((edges[n], 0.0, 0.0), (edges[n + 1], 1.0, 1.0), v, level=n // 2)
                 for n, v in enumerate(values)]
        meta = [AmrBox(b.min_corner, b.max_corner, None, b.level, dims=b.cell_dimensions)
                for b in local]
        span = ScalarTransform(normalize_to_unit_range=True, normalization_min=1.0,
                               normalization_max=21.0, inverse_normalization_span=1.0 / 20.0)
        renderer = FrameRenderer(ctx, meta, local, span, VolumeBounds(*UNIT), (0.0, 1.0))
        assert renderer.native is not None
        p = RenderParameters(W, H, 0.0, 1, draw_bounds=False)
        counter = torch.zeros(1, dtype=torch.int64, device=ctx.device)
        image, rgb8 = renderer.render(p, CAMERAS[0], samples=counter, want_image=True)
        renderer.synchronize()
        frame = [image.clone(), rgb8.clone(), int(counter.item())]
        column, length = renderer.render_projection(p, CAMERAS[0])
        renderer.synchronize()
        frame += [column.clone(), length.clone()]
        renderer.native.close()
        frames.append(frame)
    assert frames[1][2] > 0 and float(frames[1][3].max().item()) > 0.0
    image_a, image_b = frames[0][0], frames[1][0]
    assert torch.equal(image_a.view(torch.int32), image_b.view(torch.int32))
    assert_same(frames[0][1:], frames[1][1:], wide.case.name)


# ---- statistics and histograms ------------------------------------------------------------------

def test_scalar_stats_and_histogram(ctx, wide):
    every = np.concatenate([wide.host[0].reshape(-1)] +
                           [wide.small[kind][0].cpu().numpy().reshape(-1)
                            for kind in ("plain", "fine")])
    finite = every[np.isfinite(every)]
    spread = ScalarTransform(normalize_to_unit_range=True, normalization_min=1.0,
                             normalization_max=21.0, inverse_normalization_span=1.0 / 20.0)

    def run(layout, wide_first):
        scene = wide.scene(0, layout, wide_first)
        stats = scene.scalar_stats()
        counts = [scene.histogram(spread, 0.0, 1.0, bins) for bins in (64, 4097)]
        narrow = scene.histogram(NORM, 0.25, 0.75, 256)
        return stats, counts, narrow

    stats, counts, narrow = wide.read(run)
    assert stats == (float(finite.min()), float(finite.max()), float(finite.min()), finite.size)
    assert stats[1] == wide.small["fine"][0].max().item()
    for c in counts + [narrow]:
        assert int(c.sum().item()) == every.size


def test_joint_histogram(ctx, wide):
    x_edges = np.linspace(1.0, 20.0, 9)
    y_edges = np.linspace(2.0, 21.0, 6)

    def run(layout, wide_first):
        # the sums are of the field of integers: exact, whatever order the atomics take
        x, y, s = (wide.scene(f, layout, wide_first) for f in (0, 1, cases.WHOLE))
        return x.joint_histogram(x_edges, y, y_edges, s), x.joint_histogram(x_edges)

    (cells, sums, totals), (alone, _, _) = wide.read(run)
    assert int(cells.sum().item()) > 0 and int(totals[1].item()) >= 3      # NaN, +Inf, -Inf
    assert cells.shape == (2, 5, 8) and alone.shape == (2, 1, 8) and float(sums.sum().item()) > 0.0


def test_slice(ctx, wide):
    ex, ey, ez = cases.extent(wide.case)

    def run(layout, wide_first):
        scene = wide.scene(0, layout, wide_first)
        # z = 0.19 lies in plane 1 of level 0, y = 0.19 in row 1
        flat = scene.slice((0.0, 0.0, 0.19), (ex / 64, 0.0, 0.0), (0.0, ey / 16, 0.0), 64, 16)
        upright = scene.slice((0.0, 0.19, 0.0), (ex / 64, 0.0, 0.0), (0.0, 0.0, ez / 16), 64, 16)
        return flat, upright

    (value, level, box), _ = wide.read(run)
    assert int((box >= 0).sum().item()) == 64 * 16 and int(level.max().item()) == 0
    assert float(value[-1, :16].max().item()) < 2.0         # the wide box's last row of plane 1


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_axis_projection_with_and_without_a_weight(ctx, wide, axis):
    size = cases.extent(wide.case)
    eu, ev = size[(axis + 1) % 3], size[(axis + 2) % 3]

    def run(layout, wide_first):
        field, weight = wide.scene(0, layout, wide_first), wide.scene(1, layout, wide_first)
        arguments = (axis, (0.0, 0.0), eu / 32, ev / 16, 32, 16, [cases.CELL, cases.CELL / 2])
        return field.axis_projection(*arguments), field.axis_projection(*arguments, weight)

    (integral, none, length), (_, weights, _) = wide.read(run)
    assert none is None and float(length.min().item()) > 0.0 and float(weights.min().item()) > 0.0


# ---- the products that write cells --------------------------------------------------------------

PROGRAMS = ["field('a') * 2.0 + x",
            "field('a') + field('b') * field('c') - field('d') / field('e') "
            "+ minimum(field('f'), y) + z * level"]


@pytest.mark.parametrize("text", PROGRAMS, ids=["one_field", "six_fields"])
def test_derive(ctx, wide, text):
    program = api.compile_expression(text)
    n_fields = len(program.fields)
    assert n_fields == (1 if text == PROGRAMS[0] else 6)

    def run(layout, wide_first, out):
        inputs = [wide.scene(f, layout, wide_first) for f in range(n_fields)]
        origin = [cases.corners(b)[0] for b in cases.hierarchy(wide.case, wide_first)]
        out.derive(inputs, program.instructions, program.constants, origin, SIZES)

    wide.written(run)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_gradient(ctx, wide, axis):
    def run(layout, wide_first, out):
        arguments = (axis, wide.index_lo(wide_first), cases.RATIO, [cases.CELL, cases.CELL / 2])
        out.gradient(wide.scene(0, layout, wide_first), *arguments)     # with NaN / +-Inf cells
        ctx.synchronize()
        first = [b.values.clone() for b in out.boxes]
        out.gradient(wide.scene(1, layout, wide_first), *arguments)
        return first

    wide.written(run)


def test_clumps_clump_table_and_clump_links(ctx, wide):
    """The labels are written through the wide output view, and the table and the links read them
    back through it."""
    def run(layout, wide_first, out):
        index = wide.index_lo(wide_first)
        field = wide.scene(0, layout, wide_first)
        count = out.clumps(field, 1.4, 30.0, index, cases.RATIO)
        ctx.synchronize()
        n = int(count.item())
        assert n >= 1
        table = out.clump_table(n, 2, wide.scene(cases.WHOLE, layout, wide_first))  # exact sums
        links = out.clump_links(n, index, cases.RATIO)
        ctx.synchronize()
        return count, table, links

    labels, (count, table, links) = wide.written(run)
    assert max(float(t.max().item()) for t in labels) >= 1.0 and int(table[0].sum().item()) > 0


# ---- the products that look cells up ------------------------------------------------------------

def test_covering_grid(ctx, wide):
    nx, ny, nz = wide.case.view.dims

    def run(layout, wide_first):
        scene, index = wide.scene(0, layout, wide_first), wide.index_lo(wide_first)
        coarse = scene.covering_grid(0, (-1, 0, 0), (nx + cases.PLAIN_NX + 2, ny, nz), index,
                                     cases.RATIO)
        fine = scene.covering_grid(1, (0, 0, 0), (2 * (nx + cases.PLAIN_NX), 2 * ny, 2 * nz), index,
                                   cases.RATIO, fill=-1.0)
        return coarse, fine

    (values, coverage, level), (fine, _, fine_level) = wide.read(run)
    assert float(coverage[:, :, 1:-1].min().item()) == 1.0 and int(fine_level.max().item()) == 1
    # the wide box's last cell, as it is and as its eight children
    last = wide.host[0][-1, -1, -1]
    assert float(values[-1, -1, nx].item()) == last
    assert bool((fine[-2:, -2:, 2 * nx - 2:2 * nx] == last).all().item())


def test_isosurface(ctx, wide):
    def run(layout, wide_first):
        field, sample = wide.scene(1, layout, wide_first), wide.scene(2, layout, wide_first)
        arguments = (2.5, wide.index_lo(wide_first), cases.RATIO, SIZES, ORIGIN, sample)
        counts = field.isosurface(*arguments)[0]
        ctx.synchronize()
        triangles = int(counts[0].item())
        return counts, field.isosurface(*arguments, capacity=triangles)

    wide.read(run)


def test_streamlines(ctx, wide):
    ex, ey, ez = cases.extent(wide.case)
    rng = np.random.default_rng(cases.SEED)
    seeds = rng.uniform(0.02, 0.98, (24, 3)) * np.array([ex, ey, ez])
    seeds[0] = (ex - cases.PLAIN_NX * cases.CELL - 0.01, ey - 0.01, ez - 0.01)   # the last cell

    def run(layout, wide_first):
        vx, vy, vz, sample = (wide.scene(f, layout, wide_first) for f in (1, 2, 3, 4))
        index = wide.index_lo(wide_first)
        return [vx.streamlines(vy, vz, seeds, 0.5, direction, 12, index, cases.RATIO, SIZES,
                               ORIGIN, sample) for direction in (1, -1)]

    forward, backward = wide.read(run)
    assert forward[0].shape == (24, 13, 3) and backward[1].shape == (24, 13)


def _rays(case):
    ex, ey, ez = cases.extent(case)
    rng = np.random.default_rng(cases.SEED + 1)
    start = rng.uniform(-0.1, 1.1, (32, 3)) * np.array([ex, ey, ez])
    end = rng.uniform(-0.1, 1.1, (32, 3)) * np.array([ex, ey, ez])
    # along the wide box's last row, and from the first cell's corner to the last cell's
    start[0], end[0] = (-0.1, ey - 0.03, ez - 0.03), (ex + 0.1, ey - 0.03, ez - 0.03)
    start[1], end[1] = (0.0, 0.0, 0.0), (ex, ey, ez)
    return start, end


def test_rays(ctx, wide):
    start, end = _rays(wide.case)

    def run(layout, wide_first):
        scene = wide.scene(0, layout, wide_first)
        arguments = (start, end, 4096, wide.index_lo(wide_first), cases.RATIO, SIZES, ORIGIN)
        counts, status, span = scene.rays(*arguments)
        ctx.synchronize()
        offsets = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=ctx.device)
        offsets[1:] = torch.cumsum(counts.to(torch.int64), 0)
        total = int(offsets[-1].item())
        assert total > 0
        return (counts, status, span), scene.rays(*arguments, offsets=offsets, n_segments=total)

    (counts, status, _), _ = wide.read(run)
    assert int(status[0].item()) == 0 and int(counts[0].item()) >= wide.case.view.dims[0]


def test_ray_sums_with_and_without_a_weight(ctx, wide):
    start, end = _rays(wide.case)

    def run(layout, wide_first):
        field, weight = wide.scene(0, layout, wide_first), wide.scene(1, layout, wide_first)
        arguments = (start, end, 4096, wide.index_lo(wide_first), cases.RATIO, SIZES, ORIGIN)
        return field.ray_sums(*arguments), field.ray_sums(*arguments, weight=weight)

    plain, weighted = wide.read(run)
    assert plain[4] is None and float(weighted[4].max().item()) > 0.0


# ---- the products merged after this module was written -----------------------------------------

class _Scaled:
    """While it is open, one field of a case is multiplied by a power of two in every layout -- the
    view in the input storage, its contiguous copy and the ordinary boxes -- which is exact and
    exactly undone; afterwards the view holds the bits of the host's cells again."""

    def __init__(self, installed, field, factor):
        assert np.frexp(factor)[0] == 0.5
        self.installed, self.field, self.factor = installed, field, factor
        self.tensors = [installed.views[field], installed.dense[field],
                        installed.small["plain"][field], installed.small["fine"][field]]

    def __enter__(self):
        for t in self.tensors:
            t.mul_(self.factor)
        return self

    def __exit__(self, *error):
        for t in self.tensors:
            t.div_(self.factor)
        self.installed.ctx.synchronize()
        self.installed.check_storages()
        assert same_bits(self.tensors[0].cpu().numpy(), self.installed.host[self.field])
        return False


def _flat(result):
    """A result as a list of comparable pieces: tensors by their bits, on the host."""
    if isinstance(result, (tuple, list)):
        return [piece for member in result for piece in _flat(member)]
    if isinstance(result, torch.Tensor):
        t = result.contiguous().cpu()
        return [(t.view(torch.int64) if t.dtype == torch.float64 else t).numpy().tobytes()]
    return [result]


def _last_cell_pixel(case, axis, width=32, height=16):
    """(row, column) of the pixel whose line along axis crosses the wide box's last cell."""
    size = cases.extent(case)
    centre = [(n - 0.5) * cases.CELL for n in case.view.dims]
    u, v = (axis + 1) % 3, (axis + 2) % 3
    return int(centre[v] / size[v] * height), int(centre[u] / size[u] * width)


def _cube(wide, axis, emission, velocity, width_scene):
    """The window and level_dl of test_axis_projection_with_and_without_a_weight."""
    size = cases.extent(wide.case)
    eu, ev = size[(axis + 1) % 3], size[(axis + 2) % 3]
    return emission.velocity_cube(velocity, cases.CUBE_EDGES, axis, (0.0, 0.0), eu / 32, ev / 16,
                                  32, 16, [cases.CELL, cases.CELL / 2], width_scene)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_velocity_cube_sharp_and_broadened(ctx, wide, axis):
    """The slab staging and the column reads of avr_velocity_cube.hip through the views: emission
    field 0 with its NaN and infinities, velocity field 1, width field 2."""
    def run(layout, wide_first):
        emission, velocity, width = (wide.scene(f, layout, wide_first) for f in (0, 1, 2))
        return _cube(wide, axis, emission, velocity, None), _cube(wide, axis, emission, velocity,
                                                                  width)

    sharp, broadened = wide.read(run)
    row, column = _last_cell_pixel(wide.case, axis)
    for cube, under, over, length in (sharp, broadened):
        assert cube.shape == (5, 16, 32) and float(length[row, column].item()) > 0.0
    # the last cell's velocity lies in the last channel, the other boxes' above every channel; a
    # pixel stands for the line through its centre, which in the long boxes may miss the last cell
    size = cases.extent(wide.case)
    at = [(column + 0.5) * size[(axis + 1) % 3] / 32, (row + 0.5) * size[(axis + 2) % 3] / 16]
    last = [wide.case.view.dims[(axis + 1) % 3] - 1, wide.case.view.dims[(axis + 2) % 3] - 1]
    if [int(at[0] / cases.CELL), int(at[1] / cases.CELL)] == last:
        assert float(sharp[0][-1, row, column].item()) > 0.0
    assert axis != 0 or float(sharp[0][-1, row, column].item()) > 0.0     # along the last row
    assert float(sharp[1].max().item()) > 0.0 and float(sharp[2].max().item()) > 0.0


MODES = ("grey", "sharp", "broadened")


def _transfer(wide, scenes, wide_first, mode):
    """scenes: source (field 1), opacity (field 2, scaled), bin (field 3), width (field 4)."""
    source, opacity, binned, width = scenes
    start, end = _rays(wide.case)
    arguments = (start, end, 4096, wide.index_lo(wide_first), cases.RATIO, SIZES, ORIGIN)
    if mode == "grey":
        return source.ray_transfer(opacity, *arguments)
    return source.ray_transfer(opacity, *arguments, binned, width if mode == "broadened" else None,
                               cases.TRANSFER_EDGES)


def test_ray_transfer_grey_sharp_and_broadened(ctx, wide):
    """The companion-field reads of avr_rays.hip through the views; ray 0 runs along the wide box's
    last row."""
    with wide.scaled(2, cases.OPACITY_SCALE):
        def run(layout, wide_first):
            scenes = [wide.scene(f, layout, wide_first) for f in (1, 2, 3, 4)]
            return [_transfer(wide, scenes, wide_first, mode) for mode in MODES]

        results = wide.read(run)
    for mode, (counts, status, span, intensity, tau, outside, counted, covered) in zip(MODES, results):
        assert int(status[0].item()) == 0 and float(counted[0].item()) > 0.0
        assert (outside is None) == (mode == "grey")
        assert intensity.shape == ((1 if mode == "grey" else 3), 32)
        assert float(intensity[:, 0].max().item()) > 0.0
    assert 0.1 < float(results[0][4][0, 0].item()) < 10.0        # an optical depth of order 1


def _last_row(case):
    """The level-0 indices [3, nx] of the wide box's last row."""
    nx, ny, nz = case.view.dims
    return np.stack([np.arange(nx), np.full(nx, ny - 1), np.full(nx, nz - 1)]).astype(np.int64)


def _grid_fields(ctx, wide, out, wide_first, grids):
    """Every grid in every mode onto the output scene: [(the boxes' cells, totals)]."""
    results = []
    for g, device_grid in grids:
        for interpolation, periodic in g.modes:
            totals = out.grid_field(device_grid, g.level, g.lo, wide.index_lo(wide_first),
                                    cases.RATIO, interpolation, periodic)
            ctx.synchronize()
            results.append(([b.values.clone() for b in out.boxes], totals))
    return results


def test_grid_field(ctx, wide):
    """grid_tile's stores through the wide output view: a grid of the same level (the finer case for
    the fine box, constant and linear, clamped and periodic), a finer grid, and a finer grid that
    leaves fill and partial cells in the wide box."""
    grids = [(g, torch.from_numpy(g.grid).to(ctx.device)) for g in cases.wide_grids(wide.case)]
    _, results = wide.written(
        lambda layout, wide_first, out: _grid_fields(ctx, wide, out, wide_first, grids))
    # the contiguous run in the order plain, wide, fine: the wide box's last row by the reference
    nx, ny, nz = wide.case.view.dims
    runs = [(g, mode) for g, _ in grids for mode in g.modes]
    assert len(runs) == len(results) == 5
    for (g, (interpolation, periodic)), (boxes, totals) in zip(runs, results):
        want, filled, partial = grid_field_reference.grid_cells(
            g.grid, g.level, g.lo, 0, _last_row(wide.case), cases.RATIO, interpolation, periodic)
        assert same_bits(boxes[1][-1, -1, :].cpu().numpy(), want), g.name
        if g.name == "partial":
            assert filled[0] and partial[1:].all()
            assert int(totals[0].item()) >= ny * nz and int(totals[1].item()) >= (nx - 1) * ny * nz
        else:
            assert totals.tolist() == [0, 0]


def _deposit(ctx, wide, out, wide_first, points, values, method):
    found = out.particle_cells(points, values, method, wide.index_lo(wide_first), cases.RATIO,
                               SIZES, ORIGIN, levels=True)
    out.particle_deposit(found[0], found[1], 0, SIZES)
    ctx.synchronize()
    sums = [b.values.clone() for b in out.boxes]
    out.particle_deposit(found[0], found[1], 1, SIZES)
    return found, sums


@pytest.mark.parametrize("method", [0, 1])
def test_particle_cells_and_particle_deposit(ctx, wide, method):
    """clear_tile and particle_sum_kernel store through the wide output view; the cells, shares,
    levels and totals do not depend on the layout either.  The sums are in list order."""
    points, values = cases.wide_particles(wide.case)
    densities, (found, sums) = wide.written(
        lambda layout, wide_first, out: _deposit(ctx, wide, out, wide_first, points, values, method))
    nx, ny, nz = wide.case.view.dims
    h = wide_hierarchy(wide.case)       # the scene's boxes: the cells under the fine box too
    want = particle_reference.contributions(h, points, values, method)
    cells, shares, levels, totals = found
    assert totals.tolist() == [want["outside"], want["rerouted"]]
    assert same_bits(shares.cpu().numpy(), want["shares"])
    assert np.array_equal(levels.cpu().numpy(), np.where(want["leaf_level"] < 0, 255,
                                                         want["leaf_level"]))
    # the contiguous run in the order plain, wide, fine
    dense = particle_reference.deposit(h, want, 0)[0][:, :, :nx]
    got = sums[1].cpu().numpy()
    assert got.shape == dense.shape and got[-1, -1, -1] != 0.0
    assert np.array_equal(got.view(np.uint64), dense.view(np.uint64))   # +0.0 where nothing lands
    i, j, k = cases.empty_cell(wide.case)
    assert got.view(np.uint64)[k, j, i] == 0                            # the clear pass alone
    volume = (cases.CELL * cases.CELL) * cases.CELL
    assert same_bits(densities[1].cpu().numpy(), dense / volume)


def _members(ctx, wide, out, wide_first, field, sample):
    """The clumps of `field` into the output scene, their members and the members' data."""
    index = wide.index_lo(wide_first)
    count = out.clumps(field, cases.CLUMP_LOWER, cases.CLUMP_UPPER, index, cases.RATIO)
    ctx.synchronize()
    n = int(count.item())
    assert n >= 1
    cells = out.clump_table(n, 2)[0]
    ctx.synchronize()
    keys, totals = out.clump_members(n, np.ones(n, dtype=np.uint8), int(cells.sum().item()))
    data = out.clump_member_data(keys, index, cases.RATIO, SIZES, ORIGIN, field=sample)
    ctx.synchronize()
    return count, keys, totals, data


def _last_cell_ordinal(case, wide_first):
    nx, ny, nz = case.view.dims
    return (0 if wide_first else cases.PLAIN_NX * ny * nz) + nx * ny * nz - 1


def test_clump_members_and_clump_member_data(ctx, wide):
    """The labels are written through the wide output view; clump_members reads them back through
    it, and clump_member_data reads field 1 through its view."""
    def run(layout, wide_first, out):
        count, keys, totals, data = _members(ctx, wide, out, wide_first,
                                             wide.scene(0, layout, wide_first),
                                             wide.scene(1, layout, wide_first))
        at = torch.nonzero((keys & 0xffffffff) == _last_cell_ordinal(wide.case, wide_first))
        assert at.numel() == 1                                  # the last cell is a member
        return count, keys, totals, data, int(at.item())

    labels, (count, keys, totals, (levels, centres, values), at) = wide.written(run)
    assert totals.tolist() == [0] and keys.numel() > 8
    assert int(keys[at].item()) >> 32 == int(labels[1][-1, -1, -1].item()) - 1
    assert int(levels[at].item()) == 0
    assert float(values[at].item()) == wide.host[1][-1, -1, -1]
    assert centres[:, at].tolist() == [(n - 0.5) * cases.CELL for n in wide.case.view.dims]
    assert set(levels.tolist()) == {0, 1}


def test_mixed_layouts_equal_the_all_dense_run(ctx, wide):
    """Some fields are views, the others contiguous and hence paired copies: in the unpaired cases
    a product may take the pair path only if every field pairs (field_box_views)."""
    def cubes(layouts):
        emission, velocity, width = (wide.scene(f, layout) for f, layout in zip((0, 1, 2), layouts))
        out = [_cube(wide, axis, emission, velocity, width) for axis in (0, 2)]
        ctx.synchronize()
        return out

    want = cubes((False, False, False))
    for layouts in ((True, False, True), (False, True, False)):
        assert_same(cubes(layouts), want, (wide.case.name, layouts))
    with wide.scaled(2, cases.OPACITY_SCALE):
        def transfers(layouts):
            scenes = [wide.scene(f, layout) for f, layout in zip((1, 2, 3, 4), layouts)]
            out = [_transfer(wide, scenes, True, mode) for mode in MODES]
            ctx.synchronize()
            return out

        want = transfers((False, False, False, False))
        for layouts in ((True, False, True, False), (False, True, False, True)):
            assert_same(transfers(layouts), want, (wide.case.name, layouts))


def test_the_wide_boxs_last_cells_reach_every_new_product(ctx, wide):
    """So that no test above passes by never reaching the limit: on the contiguous copies alone, the
    wide box's last cell (and, where cells are read in pairs, the one before it) is replaced by
    another finite value, or the input that lands in it is, and the result must differ."""
    case = wide.case
    nx, ny, nz = case.view.dims
    cells = [(-1, -1, -1)] + ([(-1, -1, -2)] if case.others_pair else [])
    dense = [wide.scene(f, False) for f in range(5)]

    def done(result):
        ctx.synchronize()
        return _flat(result)

    # velocity_cube: the emission
    was = done(_cube(wide, 0, dense[0], dense[1], dense[2]))
    for at in cells:
        assert done(_cube(wide, 0, wide.changed_scene(0, at, 1.25), dense[1], dense[2])) != was, at
    # ray_transfer: the source, and the companion field the channels bin
    with wide.scaled(2, cases.OPACITY_SCALE):
        scenes = [wide.scene(f, False) for f in (1, 2, 3, 4)]
        was = done(_transfer(wide, scenes, True, "sharp"))
        for at in cells:
            changed = [wide.changed_scene(1, at, 2.25)] + scenes[1:]
            assert done(_transfer(wide, changed, True, "sharp")) != was, at
            changed = scenes[:2] + [wide.changed_scene(3, at, 4.375), scenes[3]]
            assert done(_transfer(wide, changed, True, "sharp")) != was, at
    # grid_field: the grid cells that land in the last cells
    margin = cases.wide_grids(case)[0]
    out, tensors = wide.output_scene(False)
    grids = [(margin._replace(modes=[(0, False)]), torch.from_numpy(margin.grid).to(ctx.device))]
    was = done(_grid_fields(ctx, wide, out, True, grids))
    for at in cells:
        grid = margin.grid.copy()
        grid[nz - 1, ny - 1, nx + 1 + at[2]] = 0.75         # the grid begins one cell below x = 0
        grids = [(margin._replace(modes=[(0, False)]), torch.from_numpy(grid).to(ctx.device))]
        now = _grid_fields(ctx, wide, out, True, grids)
        assert done(now) != was and float(now[0][0][0][at].item()) == 0.75, at
    # particles: the value of the particle in the last cell
    points, values = cases.wide_particles(case)
    was = done(_deposit(ctx, wide, out, True, points, values, 1)[1])
    values[1] = 7.0
    now = _deposit(ctx, wide, out, True, points, values, 1)[1]
    assert done(now) != was and float(now[0][-1, -1, -1].item()) != 0.0
    # clump members: the field whose value the data carry, and the field that selects the cells
    was = _members(ctx, wide, out, True, dense[0], dense[1])
    for at in cells:
        now = _members(ctx, wide, out, True, dense[0], wide.changed_scene(1, at, 2.25))
        assert _flat(now[1]) == _flat(was[1]) and _flat(now[3]) != _flat(was[3]), at
    now = _members(ctx, wide, out, True, wide.changed_scene(0, (-1, -1, -1), 1.125), dense[1])
    assert now[1].numel() == was[1].numel() - 1
    assert not bool(((now[1] & 0xffffffff) == _last_cell_ordinal(case, True)).any())
