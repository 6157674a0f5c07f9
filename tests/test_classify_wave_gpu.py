"""GPU parity of classify_wave_kernel (one wave per quarter tile, bricklet rows transposed in
registers) and of the launches that must keep to classify_kernel: every frame against the CPU
oracle, bit for bit, with an identical sample count.

The classified volume has no entry point of its own, so its bytes are checked through the march:
the images are large next to the boxes and translucent (every cell on a ray's way is sampled), and
a wrong byte is another table entry under some pixel.  The plan calls (flagged, positioned) write
send buffers, which are compared with the single-launch send buffer of the same scene; that scene's
frame is compared with the oracle here."""
import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import scenes
from amrvolumerenderer_amd.compositor import FramePlan
from amrvolumerenderer_amd.renderer import FrameRenderer, RenderParameters
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds, make_params

from helpers import (assert_bit_equal, device_box, oracle_camera, oracle_params,
                     oracle_transform)

pytestmark = pytest.mark.gpu

BOUNDS = VolumeBounds((-0.05,) * 3, (1.05,) * 3)
NORM = ScalarTransform(normalize_to_unit_range=True)
# the standard transform with a normalisation window of its own: cells 0.25 .. 0.75 -> 0 .. 1
WINDOW = ScalarTransform(normalize_to_unit_range=True, normalization_min=0.25,
                         normalization_max=0.75, inverse_normalization_span=2.0)
CAM = scenes.default_camera()
W, H = 144, 112


def random_cells(seed, nx, ny, nz):
    return np.random.default_rng(seed).random((nz, ny, nx))


def compare_box(O, ctx, cells, minc, maxc, transform=NORM, cells_view=None, transparency=0.9):
    ob = O.make_box(np.ascontiguousarray(cells), minc, maxc)
    op = oracle_params(O, W, H, (0.0, 1.0), transparency, 0.0, BOUNDS)
    want, want_n = O.paint_box(ob, oracle_transform(O, transform), op, oracle_camera(O, CAM))
    if cells_view is None:
        box = device_box(ctx, cells, minc, maxc)
    else:
        box = AmrBox(tuple(minc), tuple(maxc), cells_view)
    samples = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    got = ctx.paint_box(box, transform, make_params(W, H, (0.0, 1.0), transparency, 0.0, BOUNDS),
                        CAM, samples=samples)
    ctx.synchronize()
    assert_bit_equal(got.cpu().numpy(), want, "paint_box")
    assert int(samples.item()) == want_n and want_n > 1000
    return box


# ---- single boxes --------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", [(32, 4, 4),                       # one quarter tile exactly
                                  (64, 8, 4), (128, 4, 8), (32, 12, 20),
                                  (160, 8, 4)])                     # a last tile of one quarter
def test_boxes_of_whole_quarter_tiles(O, ctx, dims):
    nx, ny, nz = dims
    compare_box(O, ctx, random_cells(nx + ny + nz, nx, ny, nz), (0.1, 0.3, 0.35),
                (0.9, 0.3 + 0.05 * ny, 0.35 + 0.04 * nz))


def test_strided_view(O, ctx):
    """96 x 8 x 8 cut from a 128 x 16 x 16 array at an even x offset: jstride 128, kstride 2048."""
    storage = random_cells(5, 128, 16, 16)
    sl = (slice(3, 11), slice(5, 13), slice(18, 114))
    view = torch.from_numpy(storage).to(ctx.device)[sl]
    assert view.stride() == (2048, 128, 1) and view.data_ptr() % 16 == 0
    compare_box(O, ctx, storage[sl], (0.05, 0.3, 0.3), (0.95, 0.7, 0.7), cells_view=view)


def special_values():
    """Cells at the window's ends and a step outside, non-finite cells, and cells whose scaled
    float lands exactly on a table-bin edge k (and one float below and above it)."""
    values = [0.25, 0.75, np.nextafter(0.25, -1.0), np.nextafter(0.75, 2.0), np.nan, np.inf,
              -np.inf]
    on_edge = 0
    for k in (1, 2, 127, 128, 254, 255):
        f = np.float32(k / 255.0)
        for g in (np.nextafter(f, np.float32(0.0)), f, np.nextafter(f, np.float32(2.0))):
            on_edge += int(np.float32(g * np.float32(255.0)) == np.float32(k))
            values.append(0.25 + float(g) / 2.0)   # exact: (value - 0.25) * 2 is g again
            assert np.float32((values[-1] - 0.25) * 2.0) == g
    assert on_edge >= 6
    return np.array(values)


def test_special_cell_values_in_every_lane_and_plane(O, ctx):
    """Planes 0-7: the special values dealt so that each lands on every x position of a bricklet
    row (every lane of a quad, either cell of its pair) in every plane of a bricklet; planes 8-15:
    finite cells only (waves that skip the non-finite selects)."""
    special = special_values()
    nx, ny, nz = 64, 8, 16
    cells = 0.2 + 0.6 * random_cells(9, nx, ny, nz)
    z, y, x = np.meshgrid(np.arange(8), np.arange(ny), np.arange(nx), indexing="ij")
    which = (x + 3 * y + 5 * z) % len(special)
    cells[:8] = special[which]
    for s in range(len(special)):
        seen = {(int(a) % 8, int(c) % 4) for c, a in zip(z[which == s], x[which == s])}
        assert len(seen) == 32, s
    compare_box(O, ctx, cells, (0.0, 0.3, 0.2), (1.0, 0.7, 0.8), transform=WINDOW,
                transparency=0.97)


# ---- launches that keep to classify_kernel -----------------------------------------------------

def test_fallback_nx_48(O, ctx):
    compare_box(O, ctx, random_cells(48, 48, 8, 8), (0.1, 0.3, 0.3), (0.9, 0.7, 0.7))


def test_fallback_cells_offset_by_eight_bytes(O, ctx):
    storage = random_cells(6, 66, 8, 8)
    sl = (slice(0, 8), slice(0, 8), slice(1, 65))
    view = torch.from_numpy(storage).to(ctx.device)[sl]
    assert view.data_ptr() % 16 == 8
    compare_box(O, ctx, storage[sl], (0.1, 0.3, 0.3), (0.9, 0.7, 0.7), cells_view=view)


def test_fallback_log_scaled_transform(O, ctx):
    """The host's log and the device's may differ by an ulp of a double, which shows only in a cell
    whose scaled value lies that close to a table-bin edge: the thirteen values here are checked to
    lie 1e-6 of a bin or more away from every edge, so the frame is exact."""
    rng = np.random.default_rng(8)
    cells = np.exp2(rng.integers(-6, 7, size=(8, 8, 64)).astype(np.float64)) * 1.37
    lo, hi = float(np.log(2.0 ** -7)), float(np.log(2.0 ** 8))
    scaled = (np.log(np.unique(cells)) - lo) / (hi - lo) * 255.0
    assert np.abs(scaled - np.rint(scaled)).min() > 1e-6
    tr = ScalarTransform(log_scale_input=True, normalize_to_unit_range=True, positive_floor=1e-3,
                         normalization_min=lo, normalization_max=hi,
                         inverse_normalization_span=1.0 / (hi - lo))
    compare_box(O, ctx, cells, (0.1, 0.3, 0.3), (0.9, 0.7, 0.7), transform=tr)


# ---- several boxes in one launch -----------------------------------------------------------------

CORNERS = [((0.0, 0.3, 0.3), (0.6, 0.7, 0.7)), ((0.6, 0.3, 0.3), (1.0, 0.7, 0.7)),
           ((0.2, 0.7, 0.3), (0.8, 0.9, 0.7))]


def boxes_of(dims):
    return [random_cells(31 + i, *d) for i, d in enumerate(dims)]


def oracle_frame(O, cells, transparency):
    oboxes = [O.make_box(c, lo, hi) for c, (lo, hi) in zip(cells, CORNERS)]
    ref = O.reference_sample_distance(oboxes, BOUNDS.min_corner, BOUNDS.max_corner)
    op = oracle_params(O, W, H, (0.0, 1.0), transparency, ref, BOUNDS)
    ocam, otr = oracle_camera(O, CAM), oracle_transform(O, NORM)
    layers, total = [], 0
    for ob in oboxes:
        layer, n = O.paint_box(ob, otr, op, ocam)
        layers.append(layer)
        total += n
    hints = [O.box_depth_hint(ob, ocam) for ob in oboxes]
    n = len(layers)
    want, _, _ = O.compose_layered(layers, hints, [0] * n, np.arange(n, dtype=np.int32), 1)
    return want, total, ref


def renderer_frame(ctx, cells, transparency, chunks):
    local = [device_box(ctx, c, lo, hi) for c, (lo, hi) in zip(cells, CORNERS)]
    meta = [AmrBox(lo, hi, None, dims=c.shape[::-1]) for c, (lo, hi) in zip(cells, CORNERS)]
    renderer = FrameRenderer(ctx, meta, local, NORM, BOUNDS, (0.0, 1.0))
    assert renderer.native is not None
    renderer.native.set_frame_chunks(chunks)
    counter = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    image, _ = renderer.render(RenderParameters(W, H, transparency, 1, draw_bounds=False), CAM,
                               samples=counter, want_image=True)
    renderer.synchronize()
    assert renderer.native.last_frame_chunks() == chunks
    return renderer, image.cpu().numpy(), int(counter.item())


WAVE_DIMS = [(64, 8, 8), (32, 4, 12), (96, 8, 4)]


@pytest.fixture(scope="module")
def wave_scene(O):
    cells = boxes_of(WAVE_DIMS)
    return cells, oracle_frame(O, cells, 0.97)


@pytest.mark.parametrize("chunks", [1, 2])
def test_boxes_in_one_launch_and_in_two_chunks(O, ctx, wave_scene, chunks):
    """One launch: the search over the prefix sums at the boxes' boundaries; two chunks
    (avr_renderer_set_frame_chunks): a box list under each chunk's own prefix."""
    cells, (want, want_n, ref) = wave_scene
    renderer, got, counted = renderer_frame(ctx, cells, 0.97, chunks)
    assert np.float32(renderer.reference_sample_distance) == np.float32(ref)
    assert_bit_equal(got, want, f"frame in {chunks} launches")
    assert counted == want_n   # (translucent: no ray saturates, every fetch of the oracle's is made)


def test_fallback_one_box_of_the_launch_does_not_qualify(O, ctx):
    cells = boxes_of([(64, 8, 8), (48, 4, 12), (96, 8, 4)])
    want, want_n, _ = oracle_frame(O, cells, 0.97)
    _, got, counted = renderer_frame(ctx, cells, 0.97, 1)
    assert_bit_equal(got, want, "frame with a box of 48 cells")
    assert counted == want_n


def test_flagged_and_positioned_launches_over_a_poisoned_volume(O, ctx, wave_scene):
    """A flagged launch leaves the bricklets of a box with visible == 0 as they were: poison here,
    the table indices of another scalar range."""
    cells, (_, _, ref) = wave_scene
    local = [device_box(ctx, c, lo, hi) for c, (lo, hi) in zip(cells, CORNERS)]
    meta = [AmrBox(lo, hi, None, dims=c.shape[::-1]) for c, (lo, hi) in zip(cells, CORNERS)]
    scene = ctx.create_scene(local, NORM)
    plan = FramePlan(meta, make_params(W, H, (0.0, 1.0), 0.9, ref, BOUNDS), CAM, 0, 1)
    poison = FramePlan(meta, make_params(W, H, (0.2, 0.6), 0.9, ref, BOUNDS), CAM, 0, 1)
    n = max(plan.send_floats, 1)

    def march(slot):
        out = torch.full((n,), float("nan"), device=ctx.device)
        scene.march_plan(ctx, plan, slot, out)
        ctx.synchronize()
        return out.view(torch.int32)

    scene.classify_plan(ctx, plan, 0)
    want = march(0)
    flags = torch.ones(len(local), dtype=torch.uint8, device=ctx.device)
    scene.classify_plan(ctx, poison, 1)
    assert not torch.equal(march(1), want)
    scene.classify_plan_flagged(ctx, plan, 1, flags)
    assert torch.equal(march(1), want)
    for left_out in range(len(local)):   # (a position of the layer order)
        others = [p for p in range(len(local)) if p != left_out]
        flags.fill_(1)
        flags[left_out] = 0
        scene.classify_plan(ctx, poison, 1)
        scene.classify_plan_flagged(ctx, plan, 1, flags)
        flagged = march(1)
        assert not torch.equal(flagged, want), left_out    # the box is on screen, still poisoned
        scene.classify_plan(ctx, poison, 2)
        scene.classify_plan_positions(ctx, plan, 2, others)   # a launch of the others' tiles alone
        assert torch.equal(march(2), flagged), left_out
        scene.classify_plan_positions(ctx, plan, 1, [left_out])
        assert torch.equal(march(1), want), left_out
