"""Maximum-intensity projection (MIP) frames on the GPU: avr_paint_box_max, the MIP march and max
fold of avr_renderer_render_max, against the CPU oracle and against the volume frames.

The oracle has no MIP of its own.  A colour map whose table alpha is 0 below entry t and positive
from t on (a "step map") makes the oracle's volume march light a pixel exactly when some sample of
the box has index >= t: the accumulator stays 0 -- and the march unsaturated -- until that sample.
So MIP(p) = m is confirmed by "lit at t = m, dark at t = m + 1" (and -1 by "dark at t = 0"), and
an all-zero-alpha map never saturates: its fetch count is the MIP sample count."""
import os
import sys

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, scenes
from amrvolumerenderer_amd.renderer import FrameRenderer, RenderParameters
from amrvolumerenderer_amd.types import (AmrBox, CameraParameters, ColorMapControlPoint,
                                         ScalarTransform, VolumeBounds, make_params)

from helpers import (check_step_table, device_box, oracle_camera, oracle_params, oracle_transform,
                     spawn_ranks, step_map)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = VolumeBounds((-0.05,) * 3, (1.05,) * 3)
NORM = ScalarTransform(normalize_to_unit_range=True)
LAB_MAP = [(0.0, 0.0, 0.0, 0.2, 0.0), (0.25, 0.1, 0.3, 0.9, 0.1), (0.5, 0.9, 0.9, 0.2, 0.4),
           (0.8, 1.0, 0.3, 0.0, 0.7), (1.0, 1.0, 1.0, 1.0, 1.0)]


def radial(nx, ny, nz):
    x = np.arange(nx, dtype=np.float64) / max(nx - 1, 1)
    y = np.arange(ny, dtype=np.float64) / max(ny - 1, 1)
    z = np.arange(nz, dtype=np.float64) / max(nz - 1, 1)
    return np.ascontiguousarray(
        (x[None, None, :] ** 2 + y[None, :, None] ** 2 + z[:, None, None] ** 2) / 3.0)


ZERO_MAP = [(0.0, 0.5, 0.5, 0.5, 0.0), (1.0, 0.5, 0.5, 0.5, 0.0)]

def oracle_confirms_index(O, cells, minc, maxc, cam, width, height, index, samples,
                          transform=NORM, scalar_range=(0.0, 1.0), ref_dist=0.0):
    """Checks a MIP index image (row 0 at the bottom) and sample count of one box against the
    oracle's march under step maps (module docstring)."""
    ob = O.make_box(cells, minc, maxc)
    otr, ocam = oracle_transform(O, transform), oracle_camera(O, cam)

    def lit(cmap):
        op = oracle_params(O, width, height, scalar_range, 0.0, ref_dist, BOUNDS, cmap)
        img, n = O.paint_box(ob, otr, op, ocam, threads=16)
        return img[..., 3] > 0.0, n

    dark, want_samples = lit([(scalar_range[0],) + p[1:] for p in ZERO_MAP[:1]] +
                             [(scalar_range[1],) + p[1:] for p in ZERO_MAP[1:]])
    assert not dark.any()
    assert samples == want_samples, (samples, want_samples)
    distinct = sorted(int(v) for v in np.unique(index) if v >= 0)
    thresholds = sorted({0} | set(distinct) | {m + 1 for m in distinct if m < 255})
    lit_at = {}
    for t in thresholds:
        check_step_table(O, t, scalar_range)
        lit_at[t] = lit(step_map(t, scalar_range))[0]
    assert np.array_equal(index < 0, ~lit_at[0])
    for m in distinct:
        here = index == m
        assert lit_at[m][here].all(), f"MIP {m} not confirmed (oracle dark at t = {m})"
        if m < 255:
            assert not lit_at[m + 1][here].any(), f"MIP {m} too small (oracle lit at t = {m + 1})"
    return distinct


def compare_box_max(O, ctx, cells, minc, maxc, cam, width, height, transform=NORM,
                    scalar_range=(0.0, 1.0), ref_dist=0.0, color_map=None):
    box = device_box(ctx, cells, minc, maxc)
    params = make_params(width, height, scalar_range, 0.0, ref_dist, BOUNDS, color_map)
    samples = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    index = ctx.paint_box_max(box, transform, params, cam, samples=samples)
    ctx.synchronize()
    index = index.cpu().numpy()
    # the colour map does not change the index: the same image with the default map
    if color_map is not None:
        again = ctx.paint_box_max(box, transform, make_params(width, height, scalar_range, 0.0,
                                                              ref_dist, BOUNDS), cam)
        ctx.synchronize()
        assert np.array_equal(again.cpu().numpy(), index)
    return oracle_confirms_index(O, cells, minc, maxc, cam, width, height, index,
                                 int(samples.item()), transform, scalar_range, ref_dist)


# ---- single box against the oracle ----------------------------------------------------------

def test_single_box_power_of_two_spacing(O, ctx):
    distinct = compare_box_max(O, ctx, radial(32, 32, 32), (0, 0, 0), (1, 1, 1),
                               scenes.default_camera(), 96, 80, ref_dist=0.5 / 32)
    assert len(distinct) > 20


def test_single_box_reciprocal_spacing_and_custom_map(O, ctx):
    # spacings 0.7/24, 0.45/20, 1.1/36: the reciprocal index path
    compare_box_max(O, ctx, radial(24, 20, 36), (0.1, 0.2, -0.3), (0.8, 0.65, 0.8),
                    scenes.default_camera(), 80, 64, ref_dist=0.01, color_map=LAB_MAP)


def test_single_box_exact_divide_spacing(O, ctx):
    # a slab whose x extent is subnormal: 1/dx overflows, the exact IEEE divide throughout
    # (test_index_modes_gpu); a few distinct values keep the oracle's thresholds few
    rng = np.random.default_rng(5)
    cells = rng.integers(0, 6, size=(16, 16, 4)).astype(np.float64) / 5.0
    cam = CameraParameters((0.0, 0.5, 3.0), (0.0, 0.5, 0.5), (0.0, 1.0, 0.0), 30.0, 0.05, 20.0)
    distinct = compare_box_max(O, ctx, cells, (-1e-39, 0.0, 0.0), (1e-39, 1.0, 1.0), cam, 1, 64,
                               ref_dist=0.03)
    assert len(distinct) >= 2


def test_log_scale_soft_clip_and_special_cells(O, ctx):
    cells = np.exp(radial(20, 20, 20) * 6.0 - 3.0)
    flat = cells.reshape(-1)
    rng = np.random.default_rng(11)
    pick = rng.choice(flat.size, 800, replace=False)
    flat[pick[:200]] = np.nan
    flat[pick[200:300]] = np.inf
    flat[pick[300:400]] = -np.inf
    flat[pick[400:]] = -3.5                      # below the positive floor
    lo, hi = np.log(0.05), np.log(np.nanmax(cells[np.isfinite(cells)]))
    tr = ScalarTransform(log_scale_input=True, normalize_to_unit_range=True, positive_floor=0.05,
                         normalization_min=lo, normalization_max=hi,
                         inverse_normalization_span=1.0 / (hi - lo))
    # scalar range (0.1, 0.6): the soft clip of VolumePainter.cpp:723-724
    compare_box_max(O, ctx, cells, (0, 0, 0), (1, 1, 1), scenes.default_camera(), 64, 64,
                    transform=tr, scalar_range=(0.1, 0.6))


@pytest.mark.parametrize("cam", [
    CameraParameters((0.5, 0.5, 0.5), (0.9, 0.6, 0.1), (0, 1, 0), 60.0),       # eye inside the box
    CameraParameters((1.2, 1.0 + 1e-3, 0.5), (0.0, 1.0 + 1e-3, 0.5), (0, 1, 0), 50.0),  # grazing
    CameraParameters((0.5, 0.5, 3.0), (0.5, 0.5, 0.5), (0, 1, 0), 30.0),       # axis aligned
])
def test_camera_placements(O, ctx, cam):
    compare_box_max(O, ctx, radial(24, 24, 24), (0, 0, 0), (1, 1, 1), cam, 72, 56)


# ---- one-rank frames ------------------------------------------------------------------------

def _native_frame_renderer(ctx, spec, cells, color_map=None, **kwargs):
    meta = [scenes.metadata_box(spec, i) for i in range(len(cells))]
    local = [AmrBox(m.min_corner, m.max_corner, c, m.level) for c, m in zip(cells, spec.boxes)]
    cmap = None if color_map is None else [ColorMapControlPoint(*p) for p in color_map]
    renderer = FrameRenderer(ctx, meta, local, spec.transform, spec.bounds, spec.scalar_range,
                             color_map=cmap, **kwargs)
    assert renderer.native is not None
    return renderer


def rgb8_of_index(table, index):
    """Color::GetComponentAsByte of the table RGB of each index, (0, 0, 0) for -1; same rows."""
    rgb = table.reshape(256, 4)[np.clip(index, 0, 255), :3].astype(np.float32)
    byte = np.clip((rgb * np.float32(256.0)).astype(np.int32), 0, 255).astype(np.uint8)
    byte[index < 0] = 0
    return byte


@pytest.mark.parametrize("color_map", [None, LAB_MAP])
def test_one_rank_frame_is_the_max_over_boxes(O, ctx, color_map):
    spec = scenes.make_amr_scene(32, 2, 8, "smooth")
    cam = scenes.orbit_camera(3)
    W, H = 96, 64
    host = [scenes.box_cells_numpy(spec, i) for i in range(len(spec.boxes))]
    cells = [torch.from_numpy(c).to(ctx.device) for c in host]
    renderer = _native_frame_renderer(ctx, spec, cells, color_map)
    ref = renderer.reference_sample_distance
    counter = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    rgb8, index = renderer.render_max_intensity(RenderParameters(W, H, 0.0, 1, draw_bounds=False),
                                                cam, samples=counter)
    renderer.synchronize()
    rgb8, index = rgb8.cpu().numpy(), index.cpu().numpy()
    # per box: avr_paint_box_max, confirmed by the oracle; the frame is their maximum
    params = make_params(W, H, spec.scalar_range, 0.0, ref, spec.bounds, color_map)
    want = np.full((H, W), -1, np.int16)
    total = 0
    for i, (c, m) in enumerate(zip(cells, spec.boxes)):
        samples = torch.zeros(1, dtype=torch.int64, device=ctx.device)
        box_index = ctx.paint_box_max(AmrBox(m.min_corner, m.max_corner, c, m.level),
                                      spec.transform, params, cam, samples=samples)
        ctx.synchronize()
        box_index = box_index.cpu().numpy()
        if i < 4:   # (the oracle's thresholds for a few of the boxes keep the host's time short)
            oracle_confirms_index(O, host[i], m.min_corner, m.max_corner, cam, W, H, box_index,
                                  int(samples.item()), spec.transform, spec.scalar_range, ref)
        want = np.maximum(want, box_index)
        total += int(samples.item())
    assert np.array_equal(index, want)
    assert int(counter.item()) == total
    assert (index >= 0).sum() > 500 and (index < 0).sum() > 100
    # the bytes: the table RGB of the index (rows top-down), black where nothing was sampled
    table = O.build_color_table(1.0, 1.0, spec.scalar_range, color_map)
    assert np.array_equal(rgb8, rgb8_of_index(table, index)[::-1])
    assert not rgb8[::-1][index < 0].any()


@pytest.fixture(scope="module")
def config4_mip(ctx):
    spec = scenes.config4("smooth")
    cells = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
    torch.cuda.synchronize()
    renderer = _native_frame_renderer(ctx, spec, cells)
    cam = scenes.default_camera()
    rgb8, index = renderer.render_max_intensity(
        RenderParameters(2048, 2048, 0.0, 1, draw_bounds=False), cam)
    renderer.synchronize()
    index = index.cpu().numpy()
    renderer.native.close()
    return spec, cells, cam, index


def test_config4_full_size_thresholds_match_volume_frames(O, ctx, config4_mip):
    """MIP >= t exactly where the volume frame under the step map at t has alpha > 0 (the volume
    frame is the oracle-verified march, test_full_size_gpu)."""
    spec, cells, cam, index = config4_mip
    distinct = np.unique(index[index >= 0])
    assert len(distinct) > 3
    for t in (int(distinct[0]), int(distinct[len(distinct) // 2]), int(distinct[-1])):
        check_step_table(O, t, spec.scalar_range)
        renderer = _native_frame_renderer(ctx, spec, cells, step_map(t, spec.scalar_range))
        image, _ = renderer.render(RenderParameters(2048, 2048, 0.0, 1, draw_bounds=False), cam,
                                   want_image=True)
        renderer.synchronize()
        lit = image.cpu().numpy()[..., 3] > 0.0
        renderer.native.close()
        assert np.array_equal(index >= t, lit), t


# ---- volume frames are unchanged by MIP frames in between -----------------------------------

@pytest.mark.parametrize("transparency,speculation", [(0.85, 0), (0.0, 1)])
def test_volume_frames_unchanged_around_mip_frames(ctx, transparency, speculation):
    spec = scenes.make_amr_scene(32, 2, 8, "smooth")
    W, H = 120, 72
    cams = [scenes.orbit_camera(3), scenes.default_camera()]
    cells = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
    torch.cuda.synchronize()

    def run(with_mip):
        renderer = _native_frame_renderer(ctx, spec, cells)
        renderer.native.set_visibility_speculation(speculation)
        frames, mips = [], []
        for k in range(12):
            cam = cams[(k // 4) % 2]
            image, rgb8 = renderer.render(RenderParameters(W, H, transparency, 1, draw_bounds=False),
                                          cam, want_image=True)
            frames.append((image, rgb8))   # (fresh tensors per frame, read after the sync)
            if with_mip:
                mips.append(renderer.render_max_intensity(
                    RenderParameters(W, H, 0.0, 1, draw_bounds=False), cam))
        renderer.synchronize()
        state = renderer.native.speculation_state()
        renderer.native.close()
        return frames, mips, state

    plain, _, state_plain = run(False)
    mixed, mips, state_mixed = run(True)
    for (a_img, a_rgb), (b_img, b_rgb) in zip(plain, mixed):
        assert torch.equal(a_img.view(torch.int32), b_img.view(torch.int32))
        assert torch.equal(a_rgb, b_rgb)
    assert state_plain == state_mixed
    # and the MIP frames of one camera agree with each other
    assert all(torch.equal(mips[0][1], m[1]) for m in mips[:4])


# ---- errors ---------------------------------------------------------------------------------

def test_mip_frame_rejects_antialiasing_and_wireframe(ctx):
    spec = scenes.make_amr_scene(32, 1, 16, "smooth")
    cells = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
    renderer = _native_frame_renderer(ctx, spec, cells)
    cam = scenes.default_camera()
    with pytest.raises(ValueError):
        renderer.render_max_intensity(RenderParameters(64, 64, 0.0, 4, draw_bounds=False), cam)
    with pytest.raises(ValueError):
        renderer.render_max_intensity(RenderParameters(64, 64, 0.0, 1, draw_bounds=True), cam)
    # the C ABI itself
    import ctypes as C
    lib = _capi.lib()
    rgb8 = torch.empty((64, 64, 3), dtype=torch.uint8, device=ctx.device)
    for aa, bounds in ((4, 0), (1, 1)):
        rp = _capi.RenderParams(64, 64, 0.0, aa, 1, bounds, 0)
        status = lib.avr_renderer_render_max(renderer.native._handle, C.byref(rp),
                                             C.byref(cam.to_c()), None, None, None,
                                             C.c_void_p(rgb8.data_ptr()), None)
        assert status == _capi.AVR_ERR_INVALID_ARGUMENT
        assert lib.avr_last_error()
    # the renderer is still usable
    out, index = renderer.render_max_intensity(RenderParameters(64, 64, 0.0, 1, draw_bounds=False),
                                               cam)
    renderer.synchronize()
    assert (index >= 0).any()
    renderer.native.close()


# ---- N ranks on one GPU ---------------------------------------------------------------------

def _mip_worker(rank, world, port, policy, name, out_path, contiguous):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from amrvolumerenderer_amd import runtime, scenes
        from amrvolumerenderer_amd.renderer import FrameRenderer, RenderParameters
        from helpers import device_box

        W, H = 120, 73
        spec = scenes.make_amr_scene(32, 2, 8, "smooth")
        cams = [scenes.orbit_camera(3), scenes.default_camera()]
        scenes.assign_owners(spec, world, policy)
        ctx = runtime.Context(0)
        cells = [scenes.box_cells_numpy(spec, i) for i in range(len(spec.boxes))]
        meta = [scenes.metadata_box(spec, i) for i in range(len(cells))]
        local = [device_box(ctx, cells[i], spec.boxes[i].min_corner, spec.boxes[i].max_corner,
                            spec.boxes[i].level, rank)
                 for i in scenes.local_box_indices(spec, rank)]
        comm = runtime.Comm.shared(name, rank, world, 64 << 20)
        renderer = FrameRenderer(ctx, meta, local, spec.transform, spec.bounds, spec.scalar_range,
                                 rank, world, dist.group.WORLD, comm=comm)
        assert renderer.native is not None
        if contiguous:
            renderer.native.set_piece_layout(0, 1)
        p = RenderParameters(W, H, 0.0, 1, draw_bounds=False)
        # a volume frame in between: its deferred bytes ride in the MIP frame's round
        frames = [renderer.render_max_intensity(p, cams[0]),
                  renderer.render(RenderParameters(W, H, 0.85, 1, draw_bounds=False), cams[1]),
                  renderer.render_max_intensity(p, cams[1])]
        renderer.synchronize()
        if rank == 0:
            out = {}
            for k in (0, 2):
                rgb8, index = frames[k]
                out[f"rgb8_{k}"] = rgb8.cpu().numpy()
                out[f"index_{k}"] = index.cpu().numpy()
            np.savez(out_path, **out)
        else:
            assert frames[0] == (None, None) and frames[2] == (None, None)
        dist.barrier()
        renderer.native.close()
        comm.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,policy,contiguous", [(2, "morton", False), (3, "morton", False),
                                                     (3, "morton", True), (2, "level_pairs", True)])
def test_ranks_on_one_gpu_equal_the_one_rank_frame(tmp_path, ctx, world, policy, contiguous):
    out = tmp_path / "mip.npz"
    name = f"/avr_mip_{os.getpid()}_{world}_{policy}_{int(contiguous)}"
    spawn_ranks(_mip_worker, world, lambda port: (world, port, policy, name, str(out), contiguous))
    got = np.load(out)
    spec = scenes.make_amr_scene(32, 2, 8, "smooth")
    cells = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
    renderer = _native_frame_renderer(ctx, spec, cells)
    for k, cam in ((0, scenes.orbit_camera(3)), (2, scenes.default_camera())):
        rgb8, index = renderer.render_max_intensity(
            RenderParameters(120, 73, 0.0, 1, draw_bounds=False), cam)
        renderer.synchronize()
        assert np.array_equal(got[f"index_{k}"], index.cpu().numpy()), k
        assert np.array_equal(got[f"rgb8_{k}"], rgb8.cpu().numpy()), k
    renderer.native.close()
