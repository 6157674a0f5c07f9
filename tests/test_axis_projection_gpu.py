"""On-axis projections on the GPU: avr_scene_axis_projection, api.project_axis_scene and
api.project_axis against the float64 numpy reference on the plotfile's own level arrays
(axis_projection_reference).  Every cell size is a power of two, so with integer fields every
partial sum is exact and integral, weight and length must equal the reference bit for bit; with
random fields length stays exact and the sums obey the a-priori bound (2 N + 2) 2^-53 sum |term|.
Every window keeps every pixel's line at least 1e-6 of a finest cell away from every cell face
(asserted from the numpy side)."""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, plotfile
from amrvolumerenderer_amd.renderer import FrameRenderer, RenderParameters

import axis_projection_reference as ref
from helpers import colorize as _colorize
from helpers import read_png as _read_png
from helpers import spawn_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIABLES = ["density", "other", "ones"]
AXES = "xyz"


def _integers(rng, box):
    """[3, nz, ny, nx]: two fields of integers in [-1000, 1000], about 2 % of each NaN / +Inf /
    -Inf, and a field of ones."""
    lo, hi = box
    shape = (3, hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
    data = rng.integers(-1000, 1001, size=shape).astype(np.float64)
    for comp in range(2):
        flat = data[comp].reshape(-1)
        odd = rng.choice(flat.size, max(flat.size // 50, 3), replace=False)
        flat[odd] = np.array([np.nan, np.inf, -np.inf])[np.arange(odd.size) % 3]
    data[2] = 1.0
    return data


def _cells(rng, box):
    """The generator of the slice tests, plus the field of ones."""
    lo, hi = box
    shape = (3, hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
    data = rng.standard_normal(shape) * 100.0      # about half of them negative
    flat = data[:2].reshape(-1)
    odd = rng.choice(flat.size, max(flat.size // 50, 3), replace=False)
    flat[odd] = np.array([np.nan, np.inf, -np.inf])[np.arange(odd.size) % 3]
    data[:2] = flat.reshape(data[:2].shape)
    data[2] = 1.0
    return data


@dataclasses.dataclass
class Case:
    path: str
    levels: list
    lo: tuple
    hi: tuple

    def dl(self, axis):
        return [c[axis] for c in ref.cell_sizes(self.levels, self.lo, self.hi)]


def _write(path, boxes, domains, lo, hi, cells, seed):
    rng = np.random.default_rng(seed)
    levels = [{"domain": d, "boxes": b, "data": [cells(rng, box) for box in b]}
              for d, b in zip(domains, boxes)]
    plotfile.write_plotfile(str(path), VARIABLES, levels, lo, hi, [2] * (len(levels) - 1))
    return Case(str(path), levels, lo, hi)


THREE_BOXES = [
    [((0, 0, 0), (6, 9, 7)), ((7, 0, 0), (11, 9, 7))],
    [((4, 4, 2), (13, 11, 9)), ((14, 6, 4), (19, 15, 11))],
    [((12, 10, 6), (23, 19, 13)), ((30, 14, 10), (37, 25, 19))],
]
THREE_DOMAINS = [((0, 0, 0), (11, 9, 7)), ((0, 0, 0), (23, 19, 15)), ((0, 0, 0), (47, 39, 31))]
THREE_LO, THREE_HI = (0.0, -1.0, 2.0), (1.5, 0.25, 3.0)        # coarse cells of 1/8


def _three(tmp, cells, seed):
    """The slice tests' three_levels: 12 x 10 x 8 coarse cells in two grids (7 and 5 cells wide),
    two level-1 and two level-2 grids inside them, all non-cubic."""
    return _write(tmp, THREE_BOXES, THREE_DOMAINS, THREE_LO, THREE_HI, cells, seed)


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    return _three(tmp_path_factory.mktemp("axis") / "three", _integers, 2024)


@pytest.fixture(scope="module")
def three_random(tmp_path_factory):
    return _three(tmp_path_factory.mktemp("axis") / "random", _cells, 2025)


@pytest.fixture(scope="module")
def many(tmp_path_factory):
    """The slice tests' many_boxes: 16^3 coarse cells with 64 refined islands."""
    fine = [((8 * a + 2, 8 * b + 2, 8 * c + 2), (8 * a + 5, 8 * b + 5, 8 * c + 5))
            for c in range(4) for b in range(4) for a in range(4)]
    return _write(tmp_path_factory.mktemp("axis") / "many", [[((0, 0, 0), (15, 15, 15))], fine],
                  [((0, 0, 0), (15, 15, 15)), ((0, 0, 0), (31, 31, 31))],
                  (0.0, -1.0, 2.0), (1.0, 0.0, 3.0), _integers, 77)


def _one_level(tmp, axis, along, seed):
    """One level: `along` cells along the axis, 16 x 8 across it in two 8 x 8 grids."""
    au, av = ref.image_axes(axis)
    dims = [0, 0, 0]
    dims[axis], dims[au], dims[av] = along, 16, 8
    grids = []
    for half in range(2):
        lo, hi = [0, 0, 0], [d - 1 for d in dims]
        lo[au], hi[au] = 8 * half, 8 * half + 7
        grids.append((tuple(lo), tuple(hi)))
    p_lo = (0.0, -1.0, 2.0)
    p_hi = tuple(p_lo[a] + dims[a] * 0.03125 for a in range(3))
    return _write(tmp, [grids], [((0, 0, 0), tuple(d - 1 for d in dims))], p_lo, p_hi, _integers,
                  seed)


def load(ctx, case, name, min_level=0, max_level=-1):
    return plotfile.load_plotfile_geometry(ctx, case.path, name, min_level, max_level, False, True)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def window(case, axis, shift=(0.0, 0.0), zoom=(0.9237, 0.9137)):
    """A window over most of the data, off the cell faces: (center, widths)."""
    au, av = ref.image_axes(axis)
    center = [0.5 * (case.lo[a] + case.hi[a]) for a in range(3)]
    center[au] += 0.01313 * (case.hi[au] - case.lo[au]) + shift[0]
    center[av] -= 0.00917 * (case.hi[av] - case.lo[av]) - shift[1]
    return tuple(center), ((case.hi[au] - case.lo[au]) * zoom[0], (case.hi[av] - case.lo[av]) * zoom[1])


def project(ctx, case, axis, weighted, center, widths, width, height, min_level=0, max_level=-1,
            select=None, f="density", w="other"):
    """(integral, weight or None, length) as numpy, through api.project_axis_scene."""
    scenes = [load(ctx, case, name, min_level, max_level) for name in ((f, w) if weighted else (f,))]
    if select is not None:
        scenes = [dataclasses.replace(s, local_boxes=select(s.local_boxes)) for s in scenes]
    got = api.project_axis_scene(ctx, scenes[0], scenes[1] if weighted else None, AXES[axis], center,
                                 widths, width, height, case.dl(axis))
    assert got[0].shape == got[2].shape == (height, width) and got[0].dtype == torch.float64
    assert (got[1] is None) == (not weighted)
    return tuple(None if t is None else t.cpu().numpy() for t in got)


def check(ctx, case, axis, weighted, center, widths, width, height, min_level=0, max_level=-1,
          exact=True, got=None):
    assert ref.clearance(case.levels, case.lo, case.hi, center, widths, width, height, axis) >= ref.MARGIN
    want = ref.reference(case.levels, case.lo, case.hi, axis, 0, 1 if weighted else None, center,
                         widths, width, height, case.dl(axis), min_level, max_level,
                         with_fsum=not exact)
    if got is None:
        got = project(ctx, case, axis, weighted, center, widths, width, height, min_level, max_level)
    integral, weight, length = got
    assert np.array_equal(bits(length), bits(want["length"]))        # counts are exact
    if exact:
        assert np.array_equal(bits(integral), bits(want["integral"]))
        if weighted:
            assert np.array_equal(bits(weight), bits(want["weight"]))
    else:
        for name, image in (("integral", integral),) + ((("weight", weight),) if weighted else ()):
            error = np.abs(image - want[name + "_fsum"])
            limit = ref.bound(want["count"], want[name + "_abs"])
            print(name, "largest error / bound:", float((error / np.maximum(limit, 1e-300)).max()))
            assert (error <= limit).all()
    return want, got


# ---- exact cases -----------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(1, 1), (77, 53)])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_integer_fields_equal_the_reference_bit_for_bit(ctx, three, axis, weighted, size):
    center, widths = window(three, axis)
    want, _ = check(ctx, three, axis, weighted, center, widths, *size)
    if size != (1, 1):
        assert want["count"].min() > 0
        assert len(np.unique(want["count"])) > 3 and (want["integral"] != 0).sum() > 3000


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_window_partly_outside_the_data(ctx, three, axis, weighted):
    au, av = ref.image_axes(axis)
    shift = (0.41 * (three.hi[au] - three.lo[au]), 0.37 * (three.hi[av] - three.lo[av]))
    center, widths = window(three, axis, shift)
    want, got = check(ctx, three, axis, weighted, center, widths, 77, 53)
    outside = want["count"] == 0
    assert outside.sum() > 500 and (~outside).sum() > 500
    for image in got:
        assert image is None or not bits(image)[outside].any()       # +0.0


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_min_level_leaves_holes_and_max_level_zero_is_the_coarse_level(ctx, three, axis):
    center, widths = window(three, axis)
    want, _ = check(ctx, three, axis, True, center, widths, 77, 53, min_level=1)
    assert (want["count"] == 0).sum() > 300 and (want["count"] > 0).sum() > 300
    want, _ = check(ctx, three, axis, False, center, widths, 77, 53, max_level=0)
    assert want["count"].max() <= three.levels[0]["domain"][1][axis] + 1


@pytest.mark.parametrize("weighted", [False, True])
def test_more_than_two_batches_of_boxes(ctx, many, weighted):
    assert len(load(ctx, many, "density").all_boxes) > 128
    for axis in (0, 2):
        center, widths = window(many, axis)
        want, _ = check(ctx, many, axis, weighted, center, widths, 97, 61)
        assert len(np.unique(want["count"])) > 2


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_column_longer_than_a_segment_and_a_column_of_one_cell(ctx, tmp_path, axis):
    long = _one_level(tmp_path / "long", axis, 300, 5 + axis)     # 128 + 128 + 44
    flat = _one_level(tmp_path / "flat", axis, 1, 8 + axis)
    for case in (long, flat):
        assert {tuple(b.values.shape[2 - a] for a in ref.image_axes(axis))
                for b in load(ctx, case, "density").local_boxes} == {(8, 8)}
        center, widths = window(case, axis)
        for weighted in (False, True):
            want, _ = check(ctx, case, axis, weighted, center, widths, 37, 29)
            assert want["count"].max() <= (300 if case is long else 1)
    assert want["count"].max() == 1


def test_both_read_paths_are_taken(ctx, three):
    """Boxes whose cells start on a 16-byte boundary with even strides are read as f64 pairs, the
    others cell by cell: both kinds are in the scene the tests above project."""
    boxes = load(ctx, three, "density").local_boxes
    paired = [b.values.data_ptr() % 16 == 0 and b.values.stride(1) % 2 == 0 and
              b.values.stride(0) % 2 == 0 for b in boxes]
    assert any(paired) and not all(paired)
    assert any(b.values.stride(1) % 2 for b in boxes) and any(b.values.data_ptr() % 16 for b in boxes)


# ---- random fields ---------------------------------------------------------------------------------

@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_random_fields_within_the_a_priori_bound(ctx, three_random, axis, weighted):
    center, widths = window(three_random, axis)
    check(ctx, three_random, axis, weighted, center, widths, 77, 53, exact=False)


def test_two_calls_return_the_same_bits_and_a_weight_of_ones_is_the_length(ctx, three_random):
    for axis in range(3):
        center, widths = window(three_random, axis)
        first = project(ctx, three_random, axis, True, center, widths, 77, 53)
        again = project(ctx, three_random, axis, True, center, widths, 77, 53)
        for a, b in zip(first, again):
            assert np.array_equal(bits(a), bits(b))
        plain = project(ctx, three_random, axis, False, center, widths, 77, 53)
        ones = project(ctx, three_random, axis, True, center, widths, 77, 53, w="ones")
        assert np.array_equal(bits(ones[1]), bits(plain[2]))
        with np.errstate(invalid="ignore"):
            assert np.array_equal(bits(ones[0] / ones[1]), bits(plain[0] / plain[2]))


# ---- owners and ranks ------------------------------------------------------------------------------

@pytest.mark.parametrize("owners", [2, 3])
def test_owners_combine_to_the_one_owner_projection(ctx, three, three_random, owners):
    for axis in (0, 2):
        center, widths = window(three, axis)
        whole = project(ctx, three, axis, True, center, widths, 77, 53)
        parts = [project(ctx, three, axis, True, center, widths, 77, 53,
                         select=lambda boxes, o=owner: boxes[o::owners]) for owner in range(owners)]
        assert all((p[2] > 0).any() for p in parts)
        for got, want in zip(api.combine_axis_projections(parts), whole):
            assert np.array_equal(bits(got), bits(want))
        parts = [project(ctx, three_random, axis, True, center, widths, 77, 53,
                         select=lambda boxes, o=owner: boxes[o::owners]) for owner in range(owners)]
        check(ctx, three_random, axis, True, center, widths, 77, 53, exact=False,
              got=api.combine_axis_projections(parts))


def _axis_worker(rank, world, port, path, out_path, center, widths, dl):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from amrvolumerenderer_amd import api, plotfile, runtime
        ctx = runtime.Context(0)
        scenes = [plotfile.load_plotfile_geometry(ctx, path, name, 0, -1, False, True, rank, world,
                                                  dist.group.WORLD) for name in ("density", "other")]
        assert 0 < len(scenes[0].local_boxes) < len(scenes[0].all_boxes)
        got = api.project_axis_scene(ctx, scenes[0], scenes[1], "y", center, widths, 77, 53, dl,
                                     rank, world, dist.group.WORLD)
        if rank == 0:
            np.savez(out_path, integral=got[0].cpu().numpy(), weight=got[1].cpu().numpy(),
                     length=got[2].cpu().numpy())
        else:
            assert got == (None, None, None)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_equal_the_one_rank_projection(tmp_path, ctx, three):
    center, widths = window(three, 1)
    out = tmp_path / "axis.npz"
    spawn_ranks(_axis_worker, 2, lambda port: (2, port, three.path, str(out), center, widths,
                                               three.dl(1)))
    got = np.load(out)
    check(ctx, three, 1, True, center, widths, 77, 53,
          got=(got["integral"], got["weight"], got["length"]))


# ---- the C ABI's checks ----------------------------------------------------------------------------

def test_wrong_arguments_are_refused_and_the_outputs_untouched(ctx, three):
    f = load(ctx, three, "density")
    coarse = load(ctx, three, "other", 0, 0)
    sf = ctx.create_scene(f.local_boxes, f.scalar_transform)
    sw = ctx.create_scene(load(ctx, three, "other").local_boxes, f.scalar_transform)
    other = ctx.create_scene(coarse.local_boxes, coarse.scalar_transform)
    assert len(sf.boxes) != len(other.boxes)
    outs = [torch.full((5, 7), 0.5 + i, dtype=torch.float64, device=ctx.device) for i in range(3)]
    dl = three.dl(2)

    def untouched():
        ctx.synchronize()
        return all(bool((t == 0.5 + i).all()) for i, t in enumerate(outs))

    def call(scene_w, axis, origin, du, dv, width, height, level_dl, weight_out):
        level_dl = np.ascontiguousarray(level_dl, np.float64)
        return _capi.lib().avr_scene_axis_projection(
            ctx._handle, sf._handle, scene_w._handle if scene_w is not None else None, axis,
            (C.c_double * 2)(*origin), du, dv, width, height,
            level_dl.ctypes.data_as(C.POINTER(C.c_double)), level_dl.size,
            C.c_void_p(outs[0].data_ptr()),
            C.c_void_p(outs[1].data_ptr()) if weight_out else None, C.c_void_p(outs[2].data_ptr()))

    good = (sw, 2, (0.0, 0.0), 0.1, 0.1, 7, 5, dl, True)
    wrong = [
        (sw, 3, (0.0, 0.0), 0.1, 0.1, 7, 5, dl, True), (sw, -1, (0.0, 0.0), 0.1, 0.1, 7, 5, dl, True),
        (sw, 2, (0.0, 0.0), 0.1, 0.1, 0, 5, dl, True), (sw, 2, (0.0, 0.0), 0.1, 0.1, 7, -5, dl, True),
        (sw, 2, (float("nan"), 0.0), 0.1, 0.1, 7, 5, dl, True),
        (sw, 2, (0.0, 0.0), float("inf"), 0.1, 7, 5, dl, True),
        (sw, 2, (0.0, 0.0), 0.1, 0.1, 7, 5, [dl[0], float("nan"), dl[2]], True),
        (sw, 2, (0.0, 0.0), 0.1, 0.1, 7, 5, dl[:2], True),          # a box's level >= n_levels
        (sw, 2, (0.0, 0.0), 0.1, 0.1, 7, 5, [1.0] * 17, True),
        (other, 2, (0.0, 0.0), 0.1, 0.1, 7, 5, dl, True),           # another box list
        (sw, 2, (0.0, 0.0), 0.1, 0.1, 7, 5, dl, False),             # a weight scene without its image
        (None, 2, (0.0, 0.0), 0.1, 0.1, 7, 5, dl, True),            # ... and the other way round
    ]
    for arguments in wrong:
        assert call(*arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert untouched()
    with pytest.raises(ValueError, match="same number of boxes"):
        sf.axis_projection(2, (0.0, 0.0), 0.1, 0.1, 7, 5, dl, other, *outs)
    assert untouched()
    # ... and the call that is in order OVERWRITES what the arrays hold
    assert call(*good) == 0
    fresh = sf.axis_projection(2, (0.0, 0.0), 0.1, 0.1, 7, 5, dl, sw)
    ctx.synchronize()
    for got, want in zip(outs, fresh):
        assert torch.equal(got.view(torch.int64), want.view(torch.int64))
    assert not untouched()


# ---- api.project_axis ------------------------------------------------------------------------------

CMAP = [(0.0, 0.0, 0.0, 0.3, 1.0), (0.5, 0.9, 0.2, 0.1, 1.0), (1.0, 1.0, 1.0, 0.6, 1.0)]


def test_api_project_axis_returns_the_image_and_writes_the_picture(three_random, tmp_path):
    case, axis, width, height = three_random, 2, 77, 53
    au, av = ref.image_axes(axis)
    shift = (0.41 * (case.hi[au] - case.lo[au]), 0.37 * (case.hi[av] - case.lo[av]))
    center, widths = window(case, axis, shift)
    assert ref.clearance(case.levels, case.lo, case.hi, center, widths, width, height, axis) >= ref.MARGIN
    kw = dict(axis="z", width=width, height=height, center=center, plane_width=widths)
    ctx = api._runtime_scope()[0]
    table = api.projection_rgb_table(CMAP)

    plain = project(ctx, case, axis, False, center, widths, width, height)
    weighted = project(ctx, case, axis, True, center, widths, width, height)
    assert (plain[2] == 0).sum() > 500 and (plain[2] > 0).sum() > 500

    column = api.project_axis(case.path, variable="density", **kw)
    assert column.shape == (height, width) and column.dtype == np.float64
    assert np.array_equal(bits(column), bits(plain[0]))

    with np.errstate(invalid="ignore", divide="ignore"):
        want_mean = np.where(plain[2] != 0, plain[0] / plain[2], np.nan)
        want_weighted = np.where(weighted[1] != 0, weighted[0] / weighted[1], np.nan)
    mean = api.project_axis(case.path, variable="density", quantity="mean",
                            output=str(tmp_path / "mean.png"), value_range=(-60.0, 60.0),
                            color_map=CMAP, **kw)
    assert np.array_equal(np.isnan(mean), plain[2] == 0)
    assert np.array_equal(bits(mean[plain[2] != 0]), bits(want_mean[plain[2] != 0]))
    shown = plain[2] > 0
    assert np.array_equal(_read_png(tmp_path / "mean.png"),
                          _colorize(np.where(shown, want_mean, 0.0), -60.0, 60.0, table, shown))

    got = api.project_axis(case.path, variable="density", weight="other", quantity="mean", **kw)
    assert np.array_equal(np.isnan(got), weighted[1] == 0)
    keep = weighted[1] != 0
    assert np.array_equal(bits(got[keep]), bits(want_weighted[keep]))
    # ... and the sums behind them are the reference's, NaN exactly where no cell counts
    want, _ = check(ctx, case, axis, False, center, widths, width, height, exact=False, got=plain)
    assert np.array_equal(np.isnan(mean), want["length"] == 0)
    want, _ = check(ctx, case, axis, True, center, widths, width, height, exact=False, got=weighted)
    assert np.array_equal(np.isnan(got), want["count"] == 0)

    # defaults: the whole data, the first variable
    whole = api.project_axis(case.path, axis="x", width=40, height=32)
    center = tuple(0.5 * (case.lo[a] + case.hi[a]) for a in range(3))
    full = project(ctx, case, 0, False, center, (case.hi[1] - case.lo[1], case.hi[2] - case.lo[2]),
                   40, 32)
    assert np.array_equal(bits(whole), bits(full[0])) and (full[2] > 0).all()
    with pytest.raises(RuntimeError, match="not found"):
        api.project_axis(case.path, variable="density", weight="nothing", quantity="mean")


def test_slice_project_and_volume_frames_are_unchanged_around_a_project_axis(three_random, tmp_path):
    case = three_random
    ctx = api._runtime_scope()[0]
    scene = load(ctx, case, "")
    camera = api.automatic_camera(scene.bounds)
    params = RenderParameters(120, 72, 0.85, 1, draw_bounds=False)

    def frames():
        column = api.project(case.path, width=96, height=64, output=str(tmp_path / "p.png"))
        picture = _read_png(tmp_path / "p.png")
        cut = api.slice(case.path, width=64, height=48, axis="y")
        renderer = FrameRenderer(ctx, scene.all_boxes, scene.local_boxes, scene.scalar_transform,
                                 scene.bounds, scene.scalar_range)
        image, rgb8 = renderer.render(params, camera, want_image=True)
        renderer.synchronize()
        out = (column, picture, image.cpu().numpy().copy(), rgb8.cpu().numpy().copy(), cut)
        if renderer.native is not None:
            renderer.native.close()
        return out

    before = frames()
    center, widths = window(case, 0)
    image = api.project_axis(case.path, axis="x", weight="other", quantity="mean", width=77,
                             height=53, center=center, plane_width=widths,
                             output=str(tmp_path / "a.png"))
    assert np.isfinite(image).sum() > 1000
    after = frames()
    assert (before[0] != 0).sum() > 500 and before[3].any()
    assert np.array_equal(bits(before[0]), bits(after[0]))
    assert np.array_equal(before[1], after[1])
    assert np.array_equal(before[2].view(np.uint32), after[2].view(np.uint32))
    assert np.array_equal(before[3], after[3])
    assert np.array_equal(bits(before[4]), bits(after[4]))
