"""The march's four-instruction bricklet offset (IndexMode kPow2Bricks: csrc/avr_brick_address.h,
march_box in csrc/avr_kernels.hip) on the GPU, against the oracle bit for bit.

A box takes the form when its spacing is a power of two AND its y and z bricklet counts are
(pow2_brick_shifts); a launch uses it when all of its boxes do.  Every box here has corners that
are integer multiples of a power-of-two spacing, so all of them would be kPow2Multiply without the
form: the qualifying shapes (8^3, 16^3, 64^3, 20 x 16 x 13 with partial bricklets, 256 x 16 x 16
with nx at its bound, 128^3) must report mode 3 and count their samples into march counter 3, their
non-qualifying neighbours (257 x 16 x 16, 16 x 24 x 16, 16 x 17 x 16, 16 x 16 x 4, 8 x 32 x 8) must
report kPow2Multiply, and all of them must equal the oracle's layers and sample counts from four
cameras (outside, eye inside the box, grazing a face, axis-parallel) at transparencies 0, 0.5 and
0.97 -- with the sample counter (the STATS kernels) and without it.  One maximum-intensity frame of
a qualifying box, and one frame of 16^3 beside 16 x 24 x 16 through FrameRenderer, whose march must
dispatch per box (only_mode -1) and equal the oracle's composed frame."""
import numpy as np
import pytest
import torch

from amrvolumerenderer_amd.renderer import FrameRenderer, RenderParameters
from amrvolumerenderer_amd.types import (AmrBox, CameraParameters, ScalarTransform, VolumeBounds,
                                         make_params)

from helpers import (assert_bit_equal, device_box, oracle_camera, oracle_params, oracle_transform)
from test_max_intensity_gpu import LAB_MAP, compare_box_max, radial

pytestmark = pytest.mark.gpu
NORM = ScalarTransform(normalize_to_unit_range=True)
BOUNDS = VolumeBounds((-1.0,) * 3, (5.0,) * 3)
POW2_MULTIPLY, POW2_BRICKS = 0, 3      # IndexMode, csrc/avr_internal.h

# (nx, ny, nz), log2(1 / spacing), min corner in cells
QUALIFYING = [((8, 8, 8), 3, (-3, 2, -1)), ((16, 16, 16), 4, (0, 0, 0)),
              ((64, 64, 64), 6, (5, -7, 3)), ((20, 16, 13), 4, (-3, 2, -5)),
              ((256, 16, 16), 6, (-9, 4, 1)), ((128, 128, 128), 7, (11, -6, 2))]
NEIGHBOURS = [((257, 16, 16), 6, (-9, 4, 1)), ((16, 24, 16), 4, (-3, 2, -5)),
              ((16, 17, 16), 4, (1, 0, 2)), ((16, 16, 4), 4, (0, -2, 7)),
              ((8, 32, 8), 4, (2, 1, -4))]


def cameras(lo, hi):
    lo, hi = np.array(lo), np.array(hi)
    ext, centre = hi - lo, 0.5 * (lo + hi)
    size = float(np.linalg.norm(ext))
    out = {}
    direction = np.array([0.48, 0.36, 0.8])
    out["outside"] = (centre + direction * 1.6 * size, centre + 0.05 * ext, 40.0)
    eye = lo + np.array([0.3, 0.6, 0.45]) * ext
    out["inside"] = (eye, eye + np.array([0.5, -0.3, 0.8]), 80.0)
    # the eye in the plane of the +y face, looking along it: rays skim the face
    eye = centre.copy()
    eye[1] = hi[1]
    eye[0] = lo[0] - 0.5 * ext[0]
    look = centre.copy()
    look[1] = eye[1]
    out["grazing"] = (eye, look, 30.0)
    # along -z through the centre: direction components of exactly zero on the centre rays
    eye = centre.copy()
    eye[2] = hi[2] + 1.5 * ext[2]
    out["parallel"] = (eye, centre, 40.0)
    return {name: CameraParameters(tuple(float(v) for v in eye), tuple(float(v) for v in look),
                                   (0.0, 1.0, 0.0), fov, 0.05, 50.0)
            for name, (eye, look, fov) in out.items()}


def paint_and_compare(O, ctx, shape, log2_inverse, corner, want_mode):
    nx, ny, nz = shape
    h = 2.0 ** -log2_inverse
    lo = tuple(c * h for c in corner)
    hi = tuple((c + n) * h for c, n in zip(corner, shape))
    rng = np.random.default_rng(nx * 1000003 + ny * 1009 + nz)
    cells = rng.random((nz, ny, nx))
    ob = O.make_box(cells, lo, hi)
    box = device_box(ctx, cells, lo, hi)
    ref = 0.5 * h * 1.7
    W, H = 64, 56
    total, saturated = 0, False
    counters = torch.zeros(5, dtype=torch.int64, device=ctx.device)
    for name, cam in cameras(lo, hi).items():
        for transparency in (0.0, 0.5, 0.97):
            what = f"{shape} {name} {transparency}"
            # (a map that reaches alpha 1: at transparency 0 the rays saturate inside the box)
            op = oracle_params(O, W, H, (0.0, 1.0), transparency, ref, BOUNDS, LAB_MAP)
            want, want_n = O.paint_box(ob, oracle_transform(O, NORM), op, oracle_camera(O, cam))
            params = make_params(W, H, (0.0, 1.0), transparency, ref, BOUNDS, LAB_MAP)
            samples = torch.zeros(1, dtype=torch.int64, device=ctx.device)
            ctx.set_march_counters(counters)
            try:
                counted = ctx.paint_box(box, NORM, params, cam, samples=samples)
                ctx.synchronize()
            finally:
                ctx.set_march_counters(None)
            assert ctx.last_march_mode() == want_mode, what
            assert_bit_equal(counted.cpu().numpy(), want, what + " (counting)")
            assert int(samples.item()) == want_n, what
            plain = ctx.paint_box(box, NORM, params, cam)
            ctx.synchronize()
            assert ctx.last_march_mode() == want_mode, what
            assert_bit_equal(plain.cpu().numpy(), want, what)
            assert want_n > 1000, what     # the camera sees the box
            saturated = saturated or float(want[..., 3].max()) == 1.0
            total += want_n
    near, exact, reciprocal, pow2, stray = (int(v) for v in counters.cpu())
    assert (near, exact, reciprocal, stray) == (0, 0, 0, 0)
    assert pow2 == total > 50_000, (pow2, total)
    assert saturated                   # some rays ended inside the box


@pytest.mark.parametrize("shape,log2_inverse,corner", QUALIFYING,
                         ids=["x".join(map(str, s[0])) for s in QUALIFYING])
def test_qualifying_box_takes_the_form_and_matches_the_oracle(O, ctx, shape, log2_inverse, corner):
    paint_and_compare(O, ctx, shape, log2_inverse, corner, POW2_BRICKS)


@pytest.mark.parametrize("shape,log2_inverse,corner", NEIGHBOURS,
                         ids=["x".join(map(str, s[0])) for s in NEIGHBOURS])
def test_neighbouring_shape_keeps_the_general_offset(O, ctx, shape, log2_inverse, corner):
    paint_and_compare(O, ctx, shape, log2_inverse, corner, POW2_MULTIPLY)


def test_maximum_intensity_frame_of_a_qualifying_box(O, ctx):
    distinct = compare_box_max(O, ctx, radial(16, 16, 16), (0, 0, 0), (1, 1, 1),
                               CameraParameters((1.9, 1.4, 2.6), (0.5, 0.5, 0.5), (0, 1, 0), 35.0),
                               64, 56, ref_dist=0.5 / 16)
    assert ctx.last_march_mode() == POW2_BRICKS
    assert len(distinct) > 10


def frame_against_oracle(O, ctx, shapes_and_corners, h, want_mode):
    """One frame of a few boxes at spacing h through FrameRenderer against the oracle's layers,
    composed; returns nothing, asserts the image, the sample count and the march's mode."""
    W, H, transparency = 64, 56, 0.9
    bounds = VolumeBounds((-0.5,) * 3, (2.5,) * 3)
    rng = np.random.default_rng(31)
    host, lows, highs = [], [], []
    for (nx, ny, nz), corner in shapes_and_corners:
        host.append(rng.random((nz, ny, nx)))
        lows.append(tuple(c * h for c in corner))
        highs.append(tuple((c + n) * h for c, n in zip(corner, (nx, ny, nz))))
    cam = CameraParameters((3.4, 2.1, 4.0), (1.0, 0.6, 0.5), (0.0, 1.0, 0.0), 35.0, 0.05, 50.0)
    oboxes = [O.make_box(c, lo, hi) for c, lo, hi in zip(host, lows, highs)]
    ref = O.reference_sample_distance(oboxes, bounds.min_corner, bounds.max_corner)
    op = oracle_params(O, W, H, (0.0, 1.0), transparency, ref, bounds)
    ocam, otr = oracle_camera(O, cam), oracle_transform(O, NORM)
    layers, want_samples = [], 0
    for ob in oboxes:
        layer, n = O.paint_box(ob, otr, op, ocam)
        layers.append(layer)
        want_samples += n
    hints = [O.box_depth_hint(ob, ocam) for ob in oboxes]
    n = len(layers)
    want, _, _ = O.compose_layered(layers, hints, [0] * n, np.arange(n), 1)

    local = [device_box(ctx, c, lo, hi) for c, lo, hi in zip(host, lows, highs)]
    meta = [AmrBox(b.min_corner, b.max_corner, None, 0, dims=b.cell_dimensions) for b in local]
    renderer = FrameRenderer(ctx, meta, local, NORM, bounds, (0.0, 1.0))
    try:
        assert np.float32(renderer.reference_sample_distance) == np.float32(ref)
        counter = torch.zeros(1, dtype=torch.int64, device=ctx.device)
        image, _ = renderer.render(RenderParameters(W, H, transparency, 1, draw_bounds=False), cam,
                                   samples=counter, want_image=True)
        renderer.synchronize()
        assert renderer.last_march_mode() == want_mode
        assert_bit_equal(image.cpu().numpy().reshape(-1, 5), want, "frame")
        assert int(counter.item()) == want_samples > 20_000
    finally:
        if renderer.native is not None:
            renderer.native.close()


def test_mixed_scene_dispatches_per_box(O, ctx):
    # 16^3 beside 16 x 24 x 16: one box has the mode, the other does not, so the launch is not
    # specialised and the qualifying box is marched as kPow2Multiply
    frame_against_oracle(O, ctx, [((16, 16, 16), (0, 0, 0)), ((16, 24, 16), (16, 0, 0))],
                         1.0 / 16, -1)


def test_uniform_scene_is_specialised_on_the_form(O, ctx):
    frame_against_oracle(O, ctx, [((16, 16, 16), (0, 0, 0)), ((16, 16, 16), (16, 0, 0))],
                         1.0 / 16, POW2_BRICKS)
