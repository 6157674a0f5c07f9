"""The HIP march against exact ray-cell geometry (tests/continuum.py), directly: the projection,
maximum-intensity and volume kernels of one box, the frames of multi-level scenes (one rank, and
three ranks on one GPU for the projection and for the coloured volume frame) and api.project on a
written plotfile.  The coloured frames -- the march's table lookup and colour recurrence, the fold's
and the ranks' front-to-back order, the picture's bytes -- are held to the float64
emission-absorption brackets.  The cases and brackets are those of tests/test_continuum.py; nothing
here is derived from the oracle's march."""
import os

import numpy as np
import pytest
import torch

import continuum as K
import test_continuum as T
from amrvolumerenderer_amd import api, runtime, scenes
from amrvolumerenderer_amd.renderer import FrameRenderer, RenderParameters
from amrvolumerenderer_amd.types import AmrBox, ColorMapControlPoint, make_params
from helpers import SAMPLING_BOUNDS, colorize, device_box, read_png, spawn_ranks

pytestmark = pytest.mark.gpu
CMAP = [(0.0, 0.0, 0.0, 0.3, 1.0), (0.5, 0.9, 0.2, 0.1, 1.0), (1.0, 1.0, 1.0, 0.6, 1.0)]


def upload(ctx, box, cells=None):
    cells = box.cells if cells is None else cells
    return device_box(ctx, cells, box.min_corner, box.max_corner, box.level)


@pytest.mark.parametrize("name", sorted(T.SINGLE))
def test_single_box(ctx, name):
    box, cam, W, H = T.single_box(name)
    e = K.expected(cam, W, H, [box])
    params = make_params(W, H, (0.0, 1.0), 0.0, 0.0, SAMPLING_BOUNDS)
    if name == "ghost_cells_view":      # the strided view itself goes to the device
        whole = torch.from_numpy(box.cells.base).to(ctx.device)
        dbox = AmrBox(tuple(box.min_corner), tuple(box.max_corner), whole[2:-2, 2:-2, 2:-2])
    else:
        dbox = upload(ctx, box)
    column, length = ctx.paint_box_projection(dbox, params, cam)
    index = ctx.paint_box_max(upload(ctx, box, (box.index + 0.5) / 255.0), T.NORM, params, cam)
    vparams = make_params(W, H, (0.0, 1.0), 0.0, 0.0, SAMPLING_BOUNDS, T.HOMOGENEOUS_MAP)
    img = ctx.paint_box(upload(ctx, box, box.cells / 15.0), T.NORM, vparams, cam)
    ctx.synchronize()
    T.check_length_column(name, e, length.cpu().numpy(), column.cpu().numpy())
    T.check_mip(name, e, index.cpu().numpy().astype(np.int64))
    img = img.cpu().numpy().reshape(H * W, 5)
    bt = K.box_terms(cam, K.rays(cam, W, H).reshape(-1, 3), box)
    keep = ~e.excluded.reshape(-1)
    seen = (img[bt.ch.rays, 3] > 0) & keep[bt.ch.rays]
    assert seen.sum() > 200
    assert (np.abs(img[bt.ch.rays, 4].astype(np.float64) - bt.depth)[seen] <= bt.depth_margin[seen]).all()
    missed = np.ones(W * H, bool)
    missed[bt.ch.rays] = False
    assert np.isinf(img[missed & keep, 4]).all() and not img[missed & keep, 3].any()
    # the colour tables: which entry a sample takes, and the colour recurrence
    for map_name in sorted(T.COLOUR_MAPS):
        ec = T.colour_case(name, map_name)[-1]
        cparams = make_params(W, H, (0.0, 1.0), 0.0, 0.0, SAMPLING_BOUNDS, T.COLOUR_MAPS[map_name])
        if name == "ghost_cells_view":
            whole = np.full(box.cells.base.shape, 1e30)
            whole[2:-2, 2:-2, 2:-2] = T.index_cells(box)
            cbox = AmrBox(tuple(box.min_corner), tuple(box.max_corner),
                          torch.from_numpy(whole).to(ctx.device)[2:-2, 2:-2, 2:-2])
        else:
            cbox = upload(ctx, box, T.index_cells(box))
        painted = ctx.paint_box(cbox, T.NORM, cparams, cam)
        ctx.synchronize()
        T.check_colour(f"{name}/{map_name}", ec, painted.cpu().numpy().reshape(H, W, 5))


def frame_renderer(ctx, spec, boxes, cells=None, color_map=None):
    meta = [scenes.metadata_box(spec, i) for i in range(len(boxes))]
    local = [AmrBox(m.min_corner, m.max_corner,
                    torch.from_numpy(np.ascontiguousarray(b.cells if cells is None else cells(b)))
                    .to(ctx.device), m.level) for b, m in zip(boxes, spec.boxes)]
    cmap = None if color_map is None else [ColorMapControlPoint(*p) for p in color_map]
    renderer = FrameRenderer(ctx, meta, local, spec.transform, spec.bounds, spec.scalar_range,
                             color_map=cmap)
    assert renderer.native is not None
    return renderer, local


@pytest.mark.parametrize("name", sorted(T.AMR))
def test_amr_scene_frames(O, ctx, name):
    spec, cam, W, H = T.AMR[name]
    boxes = T.amr_boxes(spec, T.ramp)
    for b in boxes:
        b.index = T.mip_index(b.cells)
    plain = RenderParameters(W, H, 0.0, 1, draw_bounds=False)

    renderer, _ = frame_renderer(ctx, spec, boxes)
    column, length = renderer.render_projection(plain, cam)
    renderer.synchronize()
    column, length = column.cpu().numpy(), length.cpu().numpy()
    renderer.native.close()

    renderer, _ = frame_renderer(ctx, spec, boxes, lambda b: (b.index + 0.5) / 255.0)
    _, index = renderer.render_max_intensity(plain, cam)
    renderer.synchronize()
    index = index.cpu().numpy().astype(np.int64)
    renderer.native.close()

    transparency = 0.25
    renderer, local = frame_renderer(ctx, spec, boxes, lambda b: np.full(b.cells.shape, 0.5),
                                     T.HOMOGENEOUS_MAP)
    ref_step = float(renderer.reference_sample_distance)
    image, _ = renderer.render(RenderParameters(W, H, transparency, 1, draw_bounds=False), cam,
                               want_image=True)
    renderer.synchronize()
    alpha = image.cpu().numpy()[..., 3].astype(np.float64)
    renderer.native.close()
    # the fused paint + fold of all boxes in one run
    scene = ctx.create_scene(local, spec.transform)
    params = make_params(W, H, spec.scalar_range, transparency, ref_step, spec.bounds,
                         T.HOMOGENEOUS_MAP)
    hints = [runtime.box_depth_hint(b, cam) for b in local]
    order, run_end = runtime.layer_order(hints, [0] * len(local), list(range(len(local))))
    fused = scene.render_runs(params, cam, order, run_end, 1)
    ctx.synchronize()
    fused_alpha = fused.cpu().numpy().reshape(-1, 5)[:W * H, 3].reshape(H, W).astype(np.float64)

    per_box, a_ref = T.homogeneous_tables(O, boxes, transparency, ref_step)
    e = K.expected(cam, W, H, boxes, sample_alpha=per_box)
    T.check_length_column(name, e, length, column)
    T.check_mip(name, e, index)
    T.check_alpha(name, e, alpha, a_ref, ref_step)
    T.check_alpha(name + "_render_runs", e, fused_alpha, a_ref, ref_step)


def check_bytes(e, rgb8):
    """The picture's bytes [H, W, 3], rows top-down: each between GetComponentAsByte, int(c * 256)
    clamped to [0, 255] and so monotone in c, of the colour bracket's two ends."""
    assert rgb8.shape == e.colour.shape and rgb8.dtype == np.uint8
    as_byte = lambda c: np.clip(np.floor(c * 256.0), 0, 255).astype(np.int64)  # noqa: E731
    got = rgb8[::-1].astype(np.int64)
    ok = ~e.excluded
    assert (got >= as_byte(e.colour - e.colour_under))[ok].all()
    assert (got <= as_byte(e.colour + e.colour_over))[ok].all()
    assert not got[~e.hit & ok].any()
    assert got[e.hit].max() > 64          # a picture, not a black frame


@pytest.mark.parametrize("map_name", sorted(T.COLOUR_MAPS))
@pytest.mark.parametrize("name", sorted(T.AMR))
def test_amr_scene_frames_colour(ctx, name, map_name):
    """The coloured volume frame of render() and the fused render_runs, both transparencies."""
    spec = T.AMR[name][0]
    color_map = T.COLOUR_MAPS[map_name]
    cases = {t: T.colour_case(name, map_name, t) for t in T.TRANSPARENCIES}
    boxes, cam, W, H, ref_step = cases[T.TRANSPARENCIES[0]][:5]
    renderer, local = frame_renderer(ctx, spec, boxes, T.index_cells, color_map)
    assert float(renderer.reference_sample_distance) == ref_step
    frames = {}
    for transparency in T.TRANSPARENCIES:
        image, rgb8 = renderer.render(RenderParameters(W, H, transparency, 1, draw_bounds=False), cam,
                                      want_image=True)
        renderer.synchronize()
        frames[transparency] = (image.cpu().numpy().reshape(H, W, 5), rgb8.cpu().numpy())
    renderer.native.close()
    # the fused paint + fold of all boxes in one run
    scene = ctx.create_scene(local, spec.transform)
    hints = [runtime.box_depth_hint(b, cam) for b in local]
    order, run_end = runtime.layer_order(hints, [0] * len(local), list(range(len(local))))
    for transparency in T.TRANSPARENCIES:
        params = make_params(W, H, spec.scalar_range, transparency, ref_step, spec.bounds, color_map)
        fused = scene.render_runs(params, cam, order, run_end, 1)
        ctx.synchronize()
        e = cases[transparency][-1]
        case = f"{name}/{map_name}/{transparency}"
        T.check_colour(case + " render", e, frames[transparency][0])
        check_bytes(e, frames[transparency][1])
        T.check_colour(case + " render_runs", e,
                       fused.cpu().numpy().reshape(-1, 5)[:W * H].reshape(H, W, 5))


THREE_RANKS = "two_levels"
THREE_RANKS_COLOUR = ("contrast", 0.25)


def _three_rank_worker(rank, world, port, name, out_path):
    """One of three ranks on the one GPU: its share of the ramp scene, a projection frame."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        spec, cam, W, H = T.AMR[THREE_RANKS]
        boxes = T.amr_boxes(spec, T.ramp)
        scenes.assign_owners(spec, world, "morton")
        ctx = runtime.Context(0)
        meta = [scenes.metadata_box(spec, i) for i in range(len(boxes))]
        local = [device_box(ctx, boxes[i].cells, spec.boxes[i].min_corner, spec.boxes[i].max_corner,
                            spec.boxes[i].level, rank) for i in scenes.local_box_indices(spec, rank)]
        comm = runtime.Comm.shared(name, rank, world, 64 << 20)
        renderer = FrameRenderer(ctx, meta, local, spec.transform, spec.bounds, spec.scalar_range,
                                 rank, world, dist.group.WORLD, comm=comm)
        assert renderer.native is not None
        column, length = renderer.render_projection(RenderParameters(W, H, 0.0, 1, draw_bounds=False),
                                                    cam)
        renderer.synchronize()
        if rank == 0:
            np.savez(out_path, column=column.cpu().numpy(), length=length.cpu().numpy())
        else:
            assert column is None and length is None
        dist.barrier()
        renderer.native.close()
        comm.close()
    finally:
        dist.destroy_process_group()


def test_three_ranks_on_one_gpu_projection(tmp_path):
    """The two-level ramp scene of test_amr_scene_frames, its boxes owned by three ranks."""
    out = tmp_path / "projection.npz"
    name = f"/avr_continuum_{os.getpid()}"
    spawn_ranks(_three_rank_worker, 3, lambda port: (3, port, name, str(out)))
    got = np.load(out)
    spec, cam, W, H = T.AMR[THREE_RANKS]
    e = K.expected(cam, W, H, T.amr_boxes(spec, T.ramp))
    T.check_length_column("three_ranks", e, got["length"], got["column"])


def _three_rank_colour_worker(rank, world, port, name, out_path):
    """One of three ranks on the one GPU: its share of the scene, a coloured volume frame."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        spec, cam, W, H = T.AMR[THREE_RANKS]
        map_name, transparency = THREE_RANKS_COLOUR
        boxes = T.amr_boxes(spec, T.ramp)
        scenes.assign_owners(spec, world, "morton")
        ctx = runtime.Context(0)
        meta = [scenes.metadata_box(spec, i) for i in range(len(boxes))]
        local = [device_box(ctx, (T.mip_index(boxes[i].cells) + 0.5) / 255.0, spec.boxes[i].min_corner,
                            spec.boxes[i].max_corner, spec.boxes[i].level, rank)
                 for i in scenes.local_box_indices(spec, rank)]
        comm = runtime.Comm.shared(name, rank, world, 64 << 20)
        cmap = [ColorMapControlPoint(*p) for p in T.COLOUR_MAPS[map_name]]
        renderer = FrameRenderer(ctx, meta, local, spec.transform, spec.bounds, spec.scalar_range,
                                 rank, world, dist.group.WORLD, comm=comm, color_map=cmap)
        assert renderer.native is not None
        image, rgb8 = renderer.render(RenderParameters(W, H, transparency, 1, draw_bounds=False), cam,
                                      want_image=True)
        renderer.synchronize()
        if rank == 0:
            np.savez(out_path, image=image.cpu().numpy(), rgb8=rgb8.cpu().numpy(),
                     ref_step=float(renderer.reference_sample_distance),
                     owners=np.array([b.owner for b in spec.boxes]))
        else:
            assert image is None and rgb8 is None
        dist.barrier()
        renderer.native.close()
        comm.close()
    finally:
        dist.destroy_process_group()


def test_three_ranks_on_one_gpu_colour(tmp_path):
    """The coloured two-level scene, its boxes owned by three ranks: rank 0's frame, composited
    across the ranks, inside the brackets of the one picture."""
    out = tmp_path / "colour.npz"
    name = f"/avr_continuum_colour_{os.getpid()}"
    spawn_ranks(_three_rank_colour_worker, 3, lambda port: (3, port, name, str(out)))
    got = np.load(out)
    assert len(np.unique(got["owners"])) == 3
    map_name, transparency = THREE_RANKS_COLOUR
    _, _, W, H, ref_step, _, e = T.colour_case(THREE_RANKS, map_name, transparency)
    assert float(got["ref_step"]) == ref_step
    T.check_colour("three_ranks", e, got["image"].reshape(H, W, 5))
    check_bytes(e, got["rgb8"])


def test_config4_shape_reduced(ctx):
    """Config-4's shape (three levels, 176 boxes, the benchmark camera, a square frame) reduced to
    what the float64 traversal affords: make_amr_scene(64, 3, 16) at 256 x 256 (about 20 s of numpy
    on 16 CPUs) instead of 512^3 cells at 2048 x 2048."""
    spec = scenes.make_amr_scene(64, 3, 16)
    cam, W, H = scenes.default_camera(), 256, 256
    boxes = T.amr_boxes(spec, T.ramp)
    renderer, _ = frame_renderer(ctx, spec, boxes)
    column, length = renderer.render_projection(RenderParameters(W, H, 0.0, 1, draw_bounds=False),
                                                cam)
    renderer.synchronize()
    column, length = column.cpu().numpy(), length.cpu().numpy()
    renderer.native.close()
    T.check_length_column("config4_reduced", K.expected(cam, W, H, boxes), length, column)


def test_api_project_on_a_plotfile_is_physical_and_upright(tmp_path):
    """api.project with a camera in scene units (the loader makes the shortest edge 1) against the
    finest-value hierarchy in PHYSICAL units: world boxes, rescale, world_scale, orientation."""
    from amrvolumerenderer_amd import plotfile
    T.write_levels(tmp_path / "pf")
    pf = plotfile.PlotFileData(str(tmp_path / "pf"))
    physical, _ = T.world_boxes(pf)
    scale = 1.0 / min(T.PROB_HI)
    cam = T.PLOTFILE_CAMERA
    W, H = 64, 48
    kw = dict(width=W, height=H, camera_eye=tuple(scale * v for v in cam.eye),
              camera_look_at=tuple(scale * v for v in cam.look_at), camera_fov_y=cam.fov_y_degrees)
    column = api.project(str(tmp_path / "pf"), output=str(tmp_path / "c.png"),
                         value_range=(1.0, 60.0), color_map=CMAP, **kw)
    mean = api.project(str(tmp_path / "pf"), quantity="mean", **kw)
    e = K.expected(cam, W, H, physical)
    # the loader's own boxes, back in physical units, are the ones the brackets were made for
    # (the context api.project made on demand and keeps: the loader is asked again on that one
    # context rather than on a second one; _runtime_scope is the api module's own accessor)
    ctx = api._runtime_scope()[0]
    scene = plotfile.load_plotfile_geometry(ctx, str(tmp_path / "pf"))
    assert scene.world_scale == pytest.approx(scale, rel=1e-15)
    assert len(scene.all_boxes) == len(physical)
    for b, p in zip(scene.all_boxes, physical):
        assert np.allclose(np.array(b.min_corner) / scene.world_scale, p.min_corner, rtol=1e-14, atol=1e-14)
        assert np.allclose(np.array(b.max_corner) / scene.world_scale, p.max_corner, rtol=1e-14, atol=1e-14)
    ok = ~e.excluded
    assert e.excluded_share() <= T.MAX_EXCLUDED and e.hit.sum() > 500
    assert not (ok & e.outside("column", column)).any()
    # mean = column / length: both inside their brackets, so the quotient inside the quotients
    sampled = ok & (mean > 0)
    assert np.array_equal(mean > 0, column > 0)
    lo = (e.column - e.column_under) / np.maximum(e.length + e.length_over, 1e-300)
    hi = (e.column + e.column_over) / np.maximum(e.length - e.length_under, 1e-300)
    assert (mean[sampled] >= lo[sampled] * (1 - 1e-12)).all()
    assert (mean[sampled] <= hi[sampled] * (1 + 1e-12)).all()
    # the picture: its first row is the TOP of the scene, the array's last row
    table = api.projection_rgb_table(CMAP)
    assert np.array_equal(read_png(tmp_path / "c.png"), colorize(column, 1.0, 60.0, table))
    top, bottom = e.column[H // 2:].sum(), e.column[:H // 2].sum()
    assert abs(top - bottom) > 0.05 * (top + bottom)          # the view tells up from down
    got_top, got_bottom = column[H // 2:].sum(), column[:H // 2].sum()
    assert (got_top > got_bottom) == (top > bottom)


# physical values of the colour map's control points -> widely separated colours, so that a pixel's
# colour-table entry can be read back from its bytes (the colours themselves are not what is pinned)
MIP_MAP = [(0.0, 0.0, 0.0, 1.0, 1.0), (64.0, 0.0, 1.0, 0.0, 1.0), (128.0, 1.0, 0.0, 0.0, 1.0),
           (192.0, 1.0, 1.0, 0.0, 1.0), (255.0, 1.0, 1.0, 1.0, 1.0)]


def test_api_render_max_intensity_on_a_plotfile(tmp_path):
    """api.render(mode="max_intensity") through the loader: cells hold colour-table entry + 1/2
    under scalar_range (0, 255), so a cell's entry is floor(value) whatever the rounding; the
    picture's colours are read back as entries and held to the integer sandwich, rows top-down."""
    from amrvolumerenderer_amd import plotfile
    T.write_levels(tmp_path / "pf", lambda r: T.mip_index(r) + 0.5)
    pf = plotfile.PlotFileData(str(tmp_path / "pf"))
    physical, _ = T.world_boxes(pf)
    for b in physical:
        b.index = np.floor(b.cells).astype(np.int64)
    scale = 1.0 / min(T.PROB_HI)
    cam = T.PLOTFILE_CAMERA
    W, H = 64, 48
    out = tmp_path / "mip.png"
    assert api.render(str(tmp_path / "pf"), width=W, height=H, mode="max_intensity",
                      scalar_range=(0.0, 255.0), color_map=MIP_MAP, output=str(out),
                      camera_eye=tuple(scale * v for v in cam.eye),
                      camera_look_at=tuple(scale * v for v in cam.look_at),
                      camera_fov_y=cam.fov_y_degrees) == 0
    picture = read_png(out).astype(np.int64)
    assert picture.shape == (H, W, 3)
    # the bytes of every entry present, and black for "no sample"
    normalised = [(float(np.float32(np.float32(v) / np.float32(255.0))), r, g, b, a)
                  for v, r, g, b, a in MIP_MAP]
    table = api.projection_rgb_table(normalised).astype(np.int64)
    entries = np.array((-1,) + T.MIP_LEVELS)
    colours = np.concatenate([np.zeros((1, 3), np.int64), table[list(T.MIP_LEVELS)]])
    apart = np.abs(colours[:, None, :] - colours[None, :, :]).max(axis=-1)
    assert (apart[~np.eye(len(entries), dtype=bool)] > 40).all()
    distance = np.abs(picture[:, :, None, :] - colours[None, None, :, :]).max(axis=-1)
    assert (distance.min(axis=-1) <= 2).all()          # every pixel is one of those colours
    index = entries[distance.argmin(axis=-1)][::-1]    # the picture's first row is the scene's top
    e = K.expected(cam, W, H, physical)
    assert e.excluded_share() <= T.MAX_EXCLUDED and e.hit.sum() > 500
    T.check_mip("plotfile_max_intensity", e, index)
    assert len(np.unique(index[e.hit])) >= 3
    # upside down it would not fit
    ok = ~e.excluded
    flipped = index[::-1]
    assert ((flipped < e.mip_lo) | (flipped > e.mip_hi))[ok].mean() > 0.05
