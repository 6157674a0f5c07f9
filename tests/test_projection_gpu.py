"""Column (line-integral) projections on the GPU: avr_paint_box_projection, the projection march
and sum fold of avr_renderer_render_projection, and api.project, against the CPU oracle and
against the volume and MIP frames.

The oracle has no projection of its own, but it pins the sample set.  Paint an indicator field
(cells in {0, 1}) under a colour map whose table alpha is 0 for entry 0 and a small w for entry 255:
the oracle's pixel alpha is then the float32 recurrence a <- a + w (1 - a) applied once per sample
on a cell of value 1, strictly increasing while a < 1, so inverting it gives that count m(p)
exactly.  The all-ones field gives the number of samples n(p); the bit planes (c >> t) & 1 of
integer cells c in [0, 255] give S(p) = sum_t 2^t m_t(p).  Then length(p) = f64(step) n(p) and
column(p) = f64(step) S(p), bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import api, runtime, scenes
from amrvolumerenderer_amd.renderer import FrameRenderer, RenderParameters
from amrvolumerenderer_amd.types import (AmrBox, CameraParameters, ScalarTransform, VolumeBounds,
                                         make_params)

from helpers import colorize as _colorize
from helpers import read_png as _read_png
from helpers import count_samples, device_box, spawn_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = VolumeBounds((-0.05,) * 3, (1.05,) * 3)
NORM = ScalarTransform(normalize_to_unit_range=True)


def integer_cells(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, size=shape).astype(np.float64)


def paint(ctx, cells, minc, maxc, cam, width, height, ref_dist):
    box = device_box(ctx, cells, minc, maxc)
    params = make_params(width, height, (0.0, 1.0), 0.0, ref_dist, BOUNDS)
    samples = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    column, length = ctx.paint_box_projection(box, params, cam, samples=samples)
    ctx.synchronize()
    step = np.float64(np.float32(runtime.box_sampling(box, params)[0]))
    return column.cpu().numpy(), length.cpu().numpy(), int(samples.item()), step, box


def check_box(O, ctx, c, minc, maxc, cam, width, height, ref_dist=0.0):
    """column and length of integer cells c against the oracle's sample counts, bit for bit."""
    column, length, samples, step, box = paint(ctx, c, minc, maxc, cam, width, height, ref_dist)
    n, fetches = count_samples(O, np.ones_like(c), minc, maxc, cam, width, height, ref_dist, box)
    assert samples == fetches == int(n.sum())
    assert np.array_equal(length, step * n.astype(np.float64))
    ci = c.astype(np.int64)
    total = np.zeros((height, width), np.int64)
    for t in range(8):
        plane = ((ci >> t) & 1).astype(np.float64)
        if not plane.any():
            continue
        m, _ = count_samples(O, plane, minc, maxc, cam, width, height, ref_dist, box)
        total += m << t
    assert np.array_equal(column, step * total.astype(np.float64))
    return n


# ---- single box against the oracle, every index mode and camera placement -------------------

def test_single_box_power_of_two_spacing(O, ctx):
    n = check_box(O, ctx, integer_cells((32, 32, 32), 1), (0, 0, 0), (1, 1, 1),
                  scenes.default_camera(), 96, 64, ref_dist=0.5 / 32)
    assert (n > 0).sum() > 1000 and (n == 0).sum() > 100   # hits and misses


def test_single_box_reciprocal_spacing(O, ctx):
    check_box(O, ctx, integer_cells((36, 20, 24), 2), (0.1, 0.2, -0.3), (0.8, 0.65, 0.8),
              scenes.default_camera(), 80, 64, ref_dist=0.01)


def test_single_box_exact_divide_spacing(O, ctx):
    cam = CameraParameters((0.0, 0.5, 3.0), (0.0, 0.5, 0.5), (0.0, 1.0, 0.0), 30.0, 0.05, 20.0)
    n = check_box(O, ctx, integer_cells((16, 16, 4), 3), (-1e-39, 0.0, 0.0), (1e-39, 1.0, 1.0),
                  cam, 1, 64, ref_dist=0.03)
    assert n.sum() > 0


@pytest.mark.parametrize("cam", [
    CameraParameters((0.5, 0.5, 0.5), (0.9, 0.6, 0.1), (0, 1, 0), 60.0),       # eye inside the box
    CameraParameters((1.2, 1.0 + 1e-3, 0.5), (0.0, 1.0 + 1e-3, 0.5), (0, 1, 0), 50.0),  # grazing
    CameraParameters((0.5, 0.5, 3.0), (0.5, 0.5, 0.5), (0, 1, 0), 30.0),       # axis aligned
    CameraParameters((1.6, 0.5, 2.0), (0.9, 0.5, 0.5), (0, 1, 0), 40.0),       # partly off-screen
])
def test_camera_placements(O, ctx, cam):
    check_box(O, ctx, integer_cells((24, 24, 24), 4), (0, 0, 0), (1, 1, 1), cam, 72, 56)


def test_non_finite_cells_are_skipped_but_counted(O, ctx):
    c = integer_cells((20, 20, 20), 5)
    special = np.zeros(c.shape, bool)
    flat = special.reshape(-1)
    flat[np.random.default_rng(6).choice(flat.size, 600, replace=False)] = True
    odd = c.copy()
    values = np.array([np.nan, np.inf, -np.inf])
    odd[special] = values[np.arange(int(special.sum())) % 3]
    zeroed = c.copy()
    zeroed[special] = 0.0
    cam = scenes.default_camera()
    col_odd, len_odd, s_odd, step, box = paint(ctx, odd, (0, 0, 0), (1, 1, 1), cam, 64, 64, 0.0)
    col_zero, len_zero, s_zero, _, _ = paint(ctx, zeroed, (0, 0, 0), (1, 1, 1), cam, 64, 64, 0.0)
    hits, _ = count_samples(O, special.astype(np.float64), (0, 0, 0), (1, 1, 1), cam, 64, 64, 0.0,
                            box)
    assert hits.sum() > 0
    assert s_odd == s_zero
    assert np.array_equal(col_odd, col_zero)
    assert np.array_equal(len_odd, len_zero - step * hits.astype(np.float64))
    assert np.isfinite(col_odd).all() and np.isfinite(len_odd).all()


def test_smooth_data_is_a_sequential_sum(O, ctx):
    """Non-integer cells: the column is the f64 sum of the values over the sample set pinned
    above, to round-off -- summed from the per-cell sample counts of a separate indicator field
    per distinct value (a few values keep the oracle's work small)."""
    levels = np.array([0.1, 1.0 / 3.0, 2.7182818, 17.25])
    pick = np.random.default_rng(7).integers(0, len(levels), size=(16, 16, 16))
    cells = levels[pick]
    cam = scenes.default_camera()
    column, length, _, step, box = paint(ctx, cells, (0, 0, 0), (1, 1, 1), cam, 64, 48, 0.0)
    want = np.zeros((48, 64))
    for k, v in enumerate(levels):
        m, _ = count_samples(O, (pick == k).astype(np.float64), (0, 0, 0), (1, 1, 1), cam, 64, 48,
                             0.0, box)
        want += m * v
    want *= step
    assert np.allclose(column, want, rtol=1e-15 * 64, atol=0.0)
    assert (column > 0).sum() > 500


# ---- frames ---------------------------------------------------------------------------------

def _native_frame_renderer(ctx, spec, cells, **kwargs):
    meta = [scenes.metadata_box(spec, i) for i in range(len(cells))]
    local = [AmrBox(m.min_corner, m.max_corner, c, m.level) for c, m in zip(cells, spec.boxes)]
    renderer = FrameRenderer(ctx, meta, local, spec.transform, spec.bounds, spec.scalar_range,
                             **kwargs)
    assert renderer.native is not None
    return renderer


def scene_cells(spec, integer):
    if not integer:
        return [scenes.box_cells_numpy(spec, i) for i in range(len(spec.boxes))]
    return [integer_cells(scenes.box_cells_numpy(spec, i).shape, 100 + i)
            for i in range(len(spec.boxes))]


def per_box_sum(ctx, spec, cells, cam, width, height, ref):
    params = make_params(width, height, spec.scalar_range, 0.0, ref, spec.bounds)
    column = torch.zeros((height, width), dtype=torch.float64, device=ctx.device)
    length = torch.zeros_like(column)
    samples = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    for c, m in zip(cells, spec.boxes):
        bc, bl = ctx.paint_box_projection(AmrBox(m.min_corner, m.max_corner, c, m.level), params,
                                          cam, samples=samples)
        column += bc
        length += bl
    ctx.synchronize()
    return column.cpu().numpy(), length.cpu().numpy(), int(samples.item())


@pytest.mark.parametrize("integer", [True, False])
def test_one_rank_frame_is_the_sum_over_boxes(ctx, integer):
    spec = scenes.make_amr_scene(32, 2, 8, "smooth")
    cam = scenes.orbit_camera(3)
    W, H = 96, 64
    cells = [torch.from_numpy(c).to(ctx.device) for c in scene_cells(spec, integer)]
    renderer = _native_frame_renderer(ctx, spec, cells)
    counter = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    column, length = renderer.render_projection(RenderParameters(W, H, 0.0, 1, draw_bounds=False),
                                                cam, samples=counter)
    renderer.synchronize()
    column, length = column.cpu().numpy(), length.cpu().numpy()
    want_c, want_l, total = per_box_sum(ctx, spec, cells, cam, W, H,
                                        renderer.reference_sample_distance)
    assert int(counter.item()) == total
    assert np.array_equal(length, want_l)
    if integer:
        assert np.array_equal(column, want_c)
    else:
        assert np.allclose(column, want_c, rtol=1e-12, atol=0.0)
    assert (length > 0).sum() > 500 and (length == 0).sum() > 100
    renderer.native.close()


def test_frame_rejects_antialiasing_and_wireframe(ctx):
    import ctypes as C
    from amrvolumerenderer_amd import _capi
    spec = scenes.make_amr_scene(32, 1, 16, "smooth")
    cells = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
    renderer = _native_frame_renderer(ctx, spec, cells)
    cam = scenes.default_camera()
    with pytest.raises(ValueError):
        renderer.render_projection(RenderParameters(64, 64, 0.0, 4, draw_bounds=False), cam)
    with pytest.raises(ValueError):
        renderer.render_projection(RenderParameters(64, 64, 0.0, 1, draw_bounds=True), cam)
    out = torch.empty((2, 64, 64), dtype=torch.float64, device=ctx.device)
    for aa, bounds in ((4, 0), (1, 1)):
        rp = _capi.RenderParams(64, 64, 0.0, aa, 1, bounds, 0)
        status = _capi.lib().avr_renderer_render_projection(
            renderer.native._handle, C.byref(rp), C.byref(cam.to_c()), None, None, None,
            C.c_void_p(out[0].data_ptr()), C.c_void_p(out[1].data_ptr()))
        assert status == _capi.AVR_ERR_INVALID_ARGUMENT
    column, length = renderer.render_projection(RenderParameters(64, 64, 0.0, 1, draw_bounds=False),
                                                cam)
    renderer.synchronize()
    assert (length > 0).any()
    renderer.native.close()


def _projection_worker(rank, world, port, policy, name, out_path, contiguous):
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
        from test_projection_gpu import scene_cells

        W, H = 120, 73
        spec = scenes.make_amr_scene(32, 2, 8, "smooth")
        cams = [scenes.orbit_camera(3), scenes.default_camera()]
        scenes.assign_owners(spec, world, policy)
        ctx = runtime.Context(0)
        cells = scene_cells(spec, True)
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
        # a volume frame in between: its deferred bytes ride in the projection frame's round
        frames = [renderer.render_projection(p, cams[0]),
                  renderer.render(RenderParameters(W, H, 0.85, 1, draw_bounds=False), cams[1]),
                  renderer.render_projection(p, cams[1])]
        renderer.synchronize()
        if rank == 0:
            out = {}
            for k in (0, 2):
                column, length = frames[k]
                out[f"column_{k}"] = column.cpu().numpy()
                out[f"length_{k}"] = length.cpu().numpy()
            out["rgb8_1"] = frames[1][1].cpu().numpy()
            np.savez(out_path, **out)
        else:
            assert frames[0] == (None, None) and frames[2] == (None, None)
        dist.barrier()
        renderer.native.close()
        comm.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,policy,contiguous", [(2, "morton", False), (3, "morton", False),
                                                     (3, "morton", True)])
def test_ranks_on_one_gpu_equal_the_one_rank_frame(tmp_path, ctx, world, policy, contiguous):
    out = tmp_path / "projection.npz"
    name = f"/avr_proj_{os.getpid()}_{world}_{policy}_{int(contiguous)}"
    spawn_ranks(_projection_worker, world,
                lambda port: (world, port, policy, name, str(out), contiguous))
    got = np.load(out)
    spec = scenes.make_amr_scene(32, 2, 8, "smooth")
    cells = [torch.from_numpy(c).to(ctx.device) for c in scene_cells(spec, True)]
    renderer = _native_frame_renderer(ctx, spec, cells)
    for k, cam in ((0, scenes.orbit_camera(3)), (2, scenes.default_camera())):
        column, length = renderer.render_projection(
            RenderParameters(120, 73, 0.0, 1, draw_bounds=False), cam)
        renderer.synchronize()
        assert np.array_equal(got[f"column_{k}"], column.cpu().numpy()), k
        assert np.array_equal(got[f"length_{k}"], length.cpu().numpy()), k
    assert got["rgb8_1"].any()
    renderer.native.close()


def test_config4_full_size(ctx):
    spec = scenes.config4("smooth")
    cells = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
    torch.cuda.synchronize()
    renderer = _native_frame_renderer(ctx, spec, cells)
    cam = scenes.default_camera()
    p = RenderParameters(2048, 2048, 0.0, 1, draw_bounds=False)
    counted = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    column, length = renderer.render_projection(p, cam, samples=counted)
    mip_counted = torch.zeros(1, dtype=torch.int64, device=ctx.device)
    renderer.render_max_intensity(p, cam, samples=mip_counted)
    renderer.synchronize()
    column, length = column.cpu().numpy(), length.cpu().numpy()
    want_c, want_l, total = per_box_sum(ctx, spec, cells, cam, 2048, 2048,
                                        renderer.reference_sample_distance)
    renderer.native.close()
    assert int(counted.item()) == int(mip_counted.item()) == total
    assert np.array_equal(length, want_l)
    assert np.allclose(column, want_c, rtol=1e-12, atol=0.0)
    assert (length > 0).mean() > 0.2


def test_volume_and_mip_frames_unchanged_around_projections(ctx):
    spec = scenes.make_amr_scene(32, 2, 8, "smooth")
    W, H = 120, 72
    cams = [scenes.orbit_camera(3), scenes.default_camera()]
    cells = [scenes.box_cells_torch(spec, i, ctx.device) for i in range(len(spec.boxes))]
    torch.cuda.synchronize()

    def run(with_projection):
        renderer = _native_frame_renderer(ctx, spec, cells)
        renderer.native.set_visibility_speculation(1)
        frames, mips, projections = [], [], []
        for k in range(12):
            cam = cams[(k // 4) % 2]
            frames.append(renderer.render(RenderParameters(W, H, 0.0, 1, draw_bounds=False), cam,
                                          want_image=True))
            if with_projection:
                projections.append(renderer.render_projection(
                    RenderParameters(W, H, 0.0, 1, draw_bounds=False), cam))
            mips.append(renderer.render_max_intensity(
                RenderParameters(W, H, 0.0, 1, draw_bounds=False), cam))
            frames.append(renderer.render(RenderParameters(W, H, 0.85, 1, draw_bounds=False), cam,
                                          want_image=True))
        renderer.synchronize()
        state = renderer.native.speculation_state()
        corun = renderer.native.corun_state()
        renderer.native.close()
        return frames, mips, projections, state, corun

    plain, plain_mips, _, state_plain, corun_plain = run(False)
    mixed, mixed_mips, projections, state_mixed, corun_mixed = run(True)
    for (a_img, a_rgb), (b_img, b_rgb) in zip(plain, mixed):
        assert torch.equal(a_img.view(torch.int32), b_img.view(torch.int32))
        assert torch.equal(a_rgb, b_rgb)
    for (a_rgb, a_index), (b_rgb, b_index) in zip(plain_mips, mixed_mips):
        assert torch.equal(a_rgb, b_rgb) and torch.equal(a_index, b_index)
    assert state_plain == state_mixed
    assert corun_plain["lds_reserve_bytes"] == corun_mixed["lds_reserve_bytes"]
    # and the projections of one camera agree with each other
    assert all(torch.equal(projections[0][0], c) for c, _ in projections[:4])


# ---- api.project ----------------------------------------------------------------------------

def _write_plotfile(path, extent):
    from amrvolumerenderer_amd import plotfile
    n = 16
    data = 1.0 + np.random.default_rng(9).integers(0, 100, size=(1, n, n, n)).astype(np.float64)
    levels = [{"domain": ((0, 0, 0), (n - 1, n - 1, n - 1)),
               "boxes": [((0, 0, 0), (n - 1, n - 1, n - 1))], "data": [data]}]
    plotfile.write_plotfile(str(path), ["density"], levels, (0.0, 0.0, 0.0), (extent,) * 3, [])


CMAP = [(0.0, 0.0, 0.0, 0.3, 1.0), (0.5, 0.9, 0.2, 0.1, 1.0), (1.0, 1.0, 1.0, 0.6, 1.0)]


def test_project_scales_with_the_physical_extent_and_writes_the_picture(tmp_path):
    _write_plotfile(tmp_path / "unit", 1.0)
    _write_plotfile(tmp_path / "four", 4.0)
    kw = dict(width=96, height=64, camera_eye=(0.5, 0.7, 3.0), camera_look_at=(0.5, 0.5, 0.5))
    unit = api.project(str(tmp_path / "unit"), **kw)
    four = api.project(str(tmp_path / "four"), output=str(tmp_path / "four.png"),
                       value_range=(1.0, 300.0), color_map=CMAP, **kw)
    assert unit.shape == (64, 96) and unit.dtype == np.float64
    assert (unit > 0).sum() > 1000 and (unit == 0).sum() > 100
    assert np.array_equal(four, 4.0 * unit)
    table = api.projection_rgb_table(CMAP)
    assert np.array_equal(_read_png(tmp_path / "four.png"), _colorize(four, 1.0, 300.0, table))
    mean_unit = api.project(str(tmp_path / "unit"), quantity="mean", **kw)
    mean_four = api.project(str(tmp_path / "four"), quantity="mean", **kw)
    assert np.allclose(mean_unit, mean_four, rtol=1e-15, atol=0.0)
    assert mean_unit[mean_unit > 0].min() >= 1.0 and mean_unit.max() <= 100.0


def test_project_auto_range_and_log(tmp_path):
    _write_plotfile(tmp_path / "pf", 2.0)
    kw = dict(width=80, height=64, camera_eye=(0.5, 0.7, 3.0), camera_look_at=(0.5, 0.5, 0.5))
    table = api.projection_rgb_table(None)
    q = api.project(str(tmp_path / "pf"), output=str(tmp_path / "auto.png"), quantity="mean", **kw)
    sampled = q[q > 0]
    assert np.array_equal(_read_png(tmp_path / "auto.png"),
                          _colorize(q, sampled.min(), sampled.max(), table))
    q = api.project(str(tmp_path / "pf"), output=str(tmp_path / "log.png"), log_scale=True,
                    value_range=(0.5, 500.0), **kw)
    got = _read_png(tmp_path / "log.png")
    logq = np.log10(np.where(q > 0, q, 1.0))
    want = _colorize(logq, np.log10(0.5), np.log10(500.0), table, q > 0)
    # (the device's log10 may round differently from numpy's: a bin edge can move by an entry)
    same = np.all(got == want, axis=-1)
    assert same.mean() > 0.99
    assert np.array_equal(got[::-1][q <= 0], np.zeros_like(got[::-1][q <= 0]))
