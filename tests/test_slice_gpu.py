"""Slice images on the GPU: avr_slice_scene, avr_slice_outline, api.slice_scene and api.slice.

The reference answer is an independent float64 numpy lookup on the plotfile's own level arrays,
not on the convexified boxes: for each pixel's point, from the finest loaded level down, the first
grid whose integer index floor((P - prob_lo) / dx_l) lies inside it gives the value and the level.
That pins convexify, box ownership, the strided views into the parent grids and the kernel
together.  Every plane and image size here keeps every pixel's point at least 1e-6 of a finest
cell away from every cell face (asserted from the numpy side), so the answer does not depend on
rounding, and value (through its uint64 view), level and hit / miss must match bit for bit at
every pixel."""
import dataclasses
import os
import sys

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import api, plotfile
from amrvolumerenderer_amd.renderer import FrameRenderer, RenderParameters

from helpers import colorize as _colorize
from helpers import read_png as _read_png
from helpers import spawn_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROB_LO = (0.3, -1.1, 2.0)
PROB_HI = (1.7, 0.1, 3.05)
MARGIN = 1e-6   # of a finest cell


def _cells(rng, box, n_comp=2):
    lo, hi = box
    shape = (n_comp, hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
    data = rng.standard_normal(shape) * 100.0      # about half of them negative
    flat = data.reshape(-1)
    odd = rng.choice(flat.size, max(flat.size // 50, 3), replace=False)
    flat[odd] = np.array([np.nan, np.inf, -np.inf])[np.arange(odd.size) % 3]
    return data


def three_levels():
    """12 x 10 x 8 coarse cells in two grids, two level-1 grids and two level-2 grids inside them,
    all non-cubic: the coarse grids convexify into several sub-boxes each."""
    rng = np.random.default_rng(2024)
    boxes = [
        [((0, 0, 0), (6, 9, 7)), ((7, 0, 0), (11, 9, 7))],
        [((4, 4, 2), (13, 11, 9)), ((14, 6, 4), (19, 15, 11))],
        [((12, 10, 6), (23, 19, 13)), ((30, 14, 10), (37, 25, 19))],
    ]
    domains = [((0, 0, 0), (11, 9, 7)), ((0, 0, 0), (23, 19, 15)), ((0, 0, 0), (47, 39, 31))]
    return [{"domain": d, "boxes": b, "data": [_cells(rng, box) for box in b]}
            for d, b in zip(domains, boxes)]


def many_boxes():
    """16^3 coarse cells with 64 refined islands: far more than 64 convexified boxes."""
    rng = np.random.default_rng(77)
    coarse = [((0, 0, 0), (15, 15, 15))]
    fine = [((8 * a + 2, 8 * b + 2, 8 * c + 2), (8 * a + 5, 8 * b + 5, 8 * c + 5))
            for c in range(4) for b in range(4) for a in range(4)]
    return [{"domain": ((0, 0, 0), (15, 15, 15)), "boxes": coarse,
             "data": [_cells(rng, box) for box in coarse]},
            {"domain": ((0, 0, 0), (31, 31, 31)), "boxes": fine,
             "data": [_cells(rng, box) for box in fine]}]


def write(path, levels):
    plotfile.write_plotfile(str(path), ["density", "other"], levels, PROB_LO, PROB_HI,
                            [2] * (len(levels) - 1))
    return str(path)


def cell_sizes(levels):
    return [tuple((PROB_HI[a] - PROB_LO[a]) / (lev["domain"][1][a] - lev["domain"][0][a] + 1)
                  for a in range(3)) for lev in levels]


def basis(normal, north):
    """U = normalize(north x n), V = n x U, restated in numpy (not taken from the api)."""
    n = np.array(normal, np.float64)
    n = n / np.sqrt(n @ n)
    u = np.cross(np.array(north, np.float64), n)
    u = u / np.sqrt(u @ u)
    return n, u, np.cross(n, u)


def plane_points(plane, width, height):
    """The issue's definition, float64 numpy: P[y, x, :] in physical units."""
    _, u, v = basis(plane.normal, plane.north)
    c = np.array(plane.center, np.float64)
    s = ((np.arange(width) + 0.5) / width - 0.5) * plane.width[0]
    t = ((np.arange(height) + 0.5) / height - 0.5) * plane.width[1]
    return c + s[None, :, None] * u + t[:, None, None] * v


def assert_clear_of_faces(points, levels):
    finest = np.array(cell_sizes(levels)[-1])
    f = (points - np.array(PROB_LO)) / finest
    distance = np.abs(f - np.rint(f)).min()
    assert distance >= MARGIN, distance


def lookup(levels, points, min_level=0, max_level=-1, comp=0):
    """(value, level) per point from the level arrays, the finest loaded level first."""
    finest = len(levels) - 1
    if max_level < 0 or max_level > finest:     # -1: every level
        max_level = finest
    assert 0 <= min_level <= max_level
    value = np.zeros(points.shape[:-1], np.float64)
    level = np.full(points.shape[:-1], -1, np.int8)
    sizes = cell_sizes(levels)
    for l in range(max_level, min_level - 1, -1):
        idx = np.floor((points - np.array(PROB_LO)) / np.array(sizes[l])).astype(np.int64)
        for (lo, hi), data in zip(levels[l]["boxes"], levels[l]["data"]):
            lo, hi = np.array(lo), np.array(hi)
            inside = np.all((idx >= lo) & (idx <= hi), axis=-1) & (level < 0)
            rel = idx[inside] - lo
            value[inside] = data[comp][rel[:, 2], rel[:, 1], rel[:, 0]]
            level[inside] = l
    return value, level


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_slice(ctx, path, levels, plane, width, height, min_level=0, max_level=-1):
    points = plane_points(plane, width, height)
    assert_clear_of_faces(points, levels)
    want_value, want_level = lookup(levels, points, min_level, max_level)
    scene = plotfile.load_plotfile_geometry(ctx, path, "", min_level, max_level, False, True)
    value, level, box = api.slice_scene(ctx, scene, plane, width, height)
    assert value.shape == level.shape == box.shape == (height, width)
    value, level, box = value.cpu().numpy(), level.cpu().numpy(), box.cpu().numpy()
    assert np.array_equal(level, want_level)
    assert np.array_equal(box >= 0, want_level >= 0)
    assert np.array_equal(bits(value), bits(want_value))
    # the box image maps back: all_boxes[box] contains the point and has that level
    scaled = points * scene.world_scale
    for b in np.unique(box[box >= 0]):
        entry = scene.all_boxes[int(b)]
        mine = box == b
        assert np.all(level[mine] == entry.level)
        assert np.all((scaled[mine] >= np.array(entry.min_corner)) &
                      (scaled[mine] < np.array(entry.max_corner)))
    return scene, want_value, want_level, box


CENTER = (0.9731, -0.5213, 2.4817)
CASES = {
    "x": (api.SlicePlane((1.2345, -0.5213, 2.5171), *api.SLICE_AXES["x"], (1.1873, 1.0391)), 96, 80),
    "y": (api.SlicePlane((1.0123, -0.7321, 2.5171), *api.SLICE_AXES["y"], (1.0391, 1.3873)), 88, 96),
    "z": (api.SlicePlane((0.9731, -0.5213, 2.3391), *api.SLICE_AXES["z"], (1.3873, 1.1873)), 104, 72),
    "oblique": (api.SlicePlane(CENTER, (1.0, 0.7, 0.4), (0.0, 0.1, 1.0), (1.3171, 0.9533)), 96, 64),
    "oblique2": (api.SlicePlane(CENTER, (-0.3, 0.2, 1.0), (1.0, 1.0, 0.1), (0.8171, 1.1533)), 72, 88),
    "partly_outside": (api.SlicePlane((1.5231, -0.1213, 2.7817), (0.2, -0.1, 1.0), (0.0, 1.0, 0.0),
                                      (1.2171, 0.9533)), 80, 64),
    "one_pixel": (api.SlicePlane((1.0131, -0.4413, 2.5117), *api.SLICE_AXES["z"], (0.5, 0.5)), 1, 1),
    "odd_size": (api.SlicePlane(CENTER, (0.5, 1.0, -0.2), (0.0, 0.0, 1.0), (1.2771, 1.0133)), 77, 53),
}


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    levels = three_levels()
    return write(tmp_path_factory.mktemp("slice") / "three", levels), levels


@pytest.mark.parametrize("case", sorted(CASES))
def test_slice_equals_the_lookup_on_the_level_arrays(ctx, three, case):
    path, levels = three
    plane, width, height = CASES[case]
    scene, _, want_level, box = check_slice(ctx, path, levels, plane, width, height)
    assert len(scene.all_boxes) > 6             # the coarse grids were cut into several boxes
    if case == "partly_outside":
        assert (want_level < 0).sum() > 200 and (want_level >= 0).sum() > 200
    elif case != "one_pixel":
        assert {0, 1, 2} <= set(np.unique(want_level).tolist())
        assert len(np.unique(box)) > 6


@pytest.mark.parametrize("case", ["x", "oblique"])
def test_min_level_leaves_holes(ctx, three, case):
    path, levels = three
    plane, width, height = CASES[case]
    _, _, want_level, _ = check_slice(ctx, path, levels, plane, width, height, min_level=1)
    assert set(np.unique(want_level).tolist()) == {-1, 1, 2}


@pytest.mark.parametrize("case", ["y", "oblique2"])
def test_max_level_zero_shows_the_coarse_cells(ctx, three, case):
    path, levels = three
    plane, width, height = CASES[case]
    _, _, want_level, _ = check_slice(ctx, path, levels, plane, width, height, max_level=0)
    assert set(np.unique(want_level).tolist()) <= {-1, 0} and (want_level == 0).sum() > 1000


def test_more_than_one_batch_of_boxes(ctx, tmp_path):
    levels = many_boxes()
    path = write(tmp_path / "many", levels)
    plane = api.SlicePlane((0.9231, -0.5713, 2.4417), (0.3, -0.4, 1.0), (0.1, 1.0, 0.0),
                           (1.4171, 1.2533))
    scene, _, want_level, box = check_slice(ctx, path, levels, plane, 120, 100)
    assert len(scene.all_boxes) > 128           # three batches of 64
    assert box.max() >= 128 and len(np.unique(box)) > 30
    assert (want_level == 1).sum() > 500 and (want_level == 0).sum() > 500
    # and an axis-aligned plane through the islands
    plane = api.SlicePlane((0.9931, -0.4813, 2.1131), *api.SLICE_AXES["z"], (1.3871, 1.1933))
    _, _, want_level, _ = check_slice(ctx, path, levels, plane, 97, 61)
    assert (want_level == 1).sum() > 500


@pytest.mark.parametrize("owners", [2, 3])
def test_owners_combine_to_the_one_rank_slice(ctx, three, owners):
    path, _ = three
    scene = plotfile.load_plotfile_geometry(ctx, path, "", 0, -1, False, True)
    for case in ("oblique", "partly_outside"):
        plane, width, height = CASES[case]
        whole = api.slice_scene(ctx, scene, plane, width, height)
        parts = []
        for owner in range(owners):
            mine = dataclasses.replace(scene, local_boxes=scene.local_boxes[owner::owners])
            parts.append(api.slice_scene(ctx, mine, plane, width, height))
        hits = [int((p[1] >= 0).sum()) for p in parts]
        assert all(h > 0 for h in hits) and sum(hits) == int((whole[1] >= 0).sum())
        value, level, box = api.combine_slices(parts)
        assert torch.equal(value.view(torch.int64), whole[0].view(torch.int64))
        assert torch.equal(level, whole[1]) and torch.equal(box, whole[2])
        # ... on the host as well
        host = api.combine_slices([tuple(t.cpu().numpy() for t in p) for p in reversed(parts)])
        assert np.array_equal(bits(host[0]), bits(whole[0].cpu().numpy()))
        assert np.array_equal(host[1], whole[1].cpu().numpy())
        assert np.array_equal(host[2], whole[2].cpu().numpy())


def test_the_api_basis_is_the_numpy_restatement():
    for plane, _, _ in CASES.values():
        for got, want in zip(api.slice_basis(plane.normal, plane.north),
                             basis(plane.normal, plane.north)):
            assert np.allclose(np.array(got), want, rtol=0.0, atol=4e-16)
    n, u, v = basis((0.0, 0.0, 1.0), (0.0, 1.0, 0.0))
    assert u.tolist() == [1.0, 0.0, 0.0] and v.tolist() == [0.0, 1.0, 0.0]


def _slice_worker(rank, world, port, path, out_path, case):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from amrvolumerenderer_amd import api, plotfile, runtime
        from test_slice_gpu import CASES
        ctx = runtime.Context(0)
        scene = plotfile.load_plotfile_geometry(ctx, path, "", 0, -1, False, True, rank, world,
                                                dist.group.WORLD)
        assert 0 < len(scene.local_boxes) < len(scene.all_boxes)
        plane, width, height = CASES[case]
        got = api.slice_scene(ctx, scene, plane, width, height, rank, world, dist.group.WORLD)
        if rank == 0:
            np.savez(out_path, value=got[0].cpu().numpy(), level=got[1].cpu().numpy(),
                     box=got[2].cpu().numpy())
        else:
            assert got == (None, None, None)
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_on_one_gpu_equal_the_one_rank_slice(tmp_path, ctx, three, world):
    """slice_scene's own combine: every rank slices its boxes, a non-NCCL group stages the
    reduction of the bit patterns, levels and box indices through the host."""
    path, levels = three
    case = "partly_outside"
    out = tmp_path / "slice.npz"
    spawn_ranks(_slice_worker, world, lambda port: (world, port, path, str(out), case))
    got = np.load(out)
    plane, width, height = CASES[case]
    scene = plotfile.load_plotfile_geometry(ctx, path, "", 0, -1, False, True)
    value, level, box = api.slice_scene(ctx, scene, plane, width, height)
    assert np.array_equal(bits(got["value"]), bits(value.cpu().numpy()))
    assert got["level"].dtype == np.int8 and np.array_equal(got["level"], level.cpu().numpy())
    assert got["box"].dtype == np.int32 and np.array_equal(got["box"], box.cpu().numpy())
    want_value, want_level = lookup(levels, plane_points(plane, width, height))
    assert np.array_equal(got["level"], want_level)
    assert np.array_equal(bits(got["value"]), bits(want_value))


def outline(box, rgb, color):
    """numpy restatement of avr_slice_outline: box bottom-up, rgb top-down."""
    edge = np.zeros(box.shape, bool)
    edge[:, :-1] |= box[:, :-1] != box[:, 1:]
    edge[:-1, :] |= box[:-1, :] != box[1:, :]
    out = rgb.copy()
    out[edge[::-1]] = color
    return out, edge


def test_outline_against_numpy(ctx, three):
    path, _ = three
    scene = plotfile.load_plotfile_geometry(ctx, path, "", 0, -1, False, True)
    for case, color in (("partly_outside", (255, 255, 255)), ("odd_size", (1, 200, 33)),
                        ("one_pixel", (9, 9, 9))):
        plane, width, height = CASES[case]
        _, _, box = api.slice_scene(ctx, scene, plane, width, height)
        rgb = torch.from_numpy(np.random.default_rng(5).integers(
            0, 256, size=(height, width, 3)).astype(np.uint8)).to(ctx.device)
        before = rgb.cpu().numpy()
        ctx.slice_outline(box, rgb, color)
        ctx.synchronize()
        want, edge = outline(box.cpu().numpy(), before, color)
        assert np.array_equal(rgb.cpu().numpy(), want)
        assert edge.any() == (case != "one_pixel")
    with pytest.raises(ValueError):
        ctx.slice_outline(box, rgb[..., :2].contiguous())
    with pytest.raises(ValueError):
        ctx.slice_outline(box.to(torch.int64), rgb)
    with pytest.raises(ValueError):
        ctx.slice_outline(box, rgb, (0, 0, 256))


CMAP = [(0.0, 0.0, 0.0, 0.3, 1.0), (0.5, 0.9, 0.2, 0.1, 1.0), (1.0, 1.0, 1.0, 0.6, 1.0)]


def test_api_slice_returns_the_image_and_writes_the_picture(three, tmp_path):
    path, levels = three
    plane, width, height = CASES["z"]
    kw = dict(width=width, height=height, center=plane.center, normal=plane.normal,
              north=plane.north, plane_width=plane.width)
    points = plane_points(plane, width, height)
    assert_clear_of_faces(points, levels)
    want_value, want_level = lookup(levels, points, comp=1)
    hit = want_level >= 0
    table = api.projection_rgb_table(CMAP)

    image = api.slice(path, variable="other", output=str(tmp_path / "fixed.png"),
                      value_range=(-150.0, 250.0), color_map=CMAP, **kw)
    assert image.shape == (height, width) and image.dtype == np.float64
    assert np.array_equal(np.isnan(image), ~hit | np.isnan(want_value))
    assert np.array_equal(bits(image[hit]), bits(want_value[hit]))
    shown = hit & np.isfinite(want_value)
    assert (~shown & hit).any()                         # NaN / Inf cells are in the picture's plane
    q = np.where(shown, want_value, 0.0)
    got = _read_png(tmp_path / "fixed.png")
    assert np.array_equal(got, _colorize(q, -150.0, 250.0, table, shown))
    assert not got[::-1][~hit].any()                    # misses are black

    # automatic range = min and max of the finite hits; outlines in white on top
    api.slice(path, variable="other", output=str(tmp_path / "auto.png"), annotate_grids=True, **kw)
    ctx = api._runtime_scope()[0]
    scene = plotfile.load_plotfile_geometry(ctx, path, "other", 0, -1, False, True)
    box = api.slice_scene(ctx, scene, plane, width, height)[2].cpu().numpy()
    plain = _colorize(q, q[shown].min(), q[shown].max(), api.projection_rgb_table(None), shown)
    want, edge = outline(box, plain, (255, 255, 255))
    assert edge.sum() > 100
    assert np.array_equal(_read_png(tmp_path / "auto.png"), want)

    # the level picture, as a PPM
    levels_image = api.slice(path, quantity="level", output=str(tmp_path / "level.ppm"),
                             value_range=(0.0, 2.0), **kw)
    assert np.array_equal(np.isnan(levels_image), ~hit)
    assert np.array_equal(levels_image[hit], want_level[hit].astype(np.float64))
    raw = open(tmp_path / "level.ppm", "rb").read()
    head = f"P6\n{width} {height}\n255\n".encode()
    assert raw.startswith(head)
    got = np.frombuffer(raw[len(head):], np.uint8).reshape(height, width, 3)
    want = _colorize(np.where(hit, want_level, 0).astype(np.float64), 0.0, 2.0,
                     api.projection_rgb_table(None), hit)
    assert np.array_equal(got, want)


def test_api_slice_defaults_cover_the_data(three):
    path, levels = three
    # 96 x 80 pixels over 48 x 40 finest cells: two pixels per cell, centres on the quarters;
    # the default centre lies on a cell face along z, so the plane is moved off it
    center = tuple(0.5 * (PROB_LO[a] + PROB_HI[a]) for a in range(3))
    image = api.slice(path, width=96, height=80, axis="z", center=center[:2] + (2.5171,))
    plane = api.SlicePlane(center[:2] + (2.5171,), *api.SLICE_AXES["z"],
                           (PROB_HI[0] - PROB_LO[0], PROB_HI[1] - PROB_LO[1]))
    points = plane_points(plane, 96, 80)
    assert_clear_of_faces(points, levels)
    want_value, want_level = lookup(levels, points)
    assert (want_level >= 0).all()
    assert np.array_equal(bits(image), bits(want_value))


def test_project_and_volume_frames_are_unchanged_around_a_slice(three, tmp_path):
    path, _ = three
    ctx = api._runtime_scope()[0]
    scene = plotfile.load_plotfile_geometry(ctx, path, "", 0, -1, False, True)
    camera = api.automatic_camera(scene.bounds)
    params = RenderParameters(120, 72, 0.85, 1, draw_bounds=False)

    def frames():
        column = api.project(path, width=96, height=64, output=str(tmp_path / "p.png"))
        picture = _read_png(tmp_path / "p.png")
        renderer = FrameRenderer(ctx, scene.all_boxes, scene.local_boxes, scene.scalar_transform,
                                 scene.bounds, scene.scalar_range)
        image, rgb8 = renderer.render(params, camera, want_image=True)
        renderer.synchronize()
        out = (column, picture, image.cpu().numpy().copy(), rgb8.cpu().numpy().copy())
        if renderer.native is not None:
            renderer.native.close()
        return out

    before = frames()
    plane, width, height = CASES["oblique"]
    image = api.slice(path, width=width, height=height, center=plane.center, normal=plane.normal,
                      north=plane.north, plane_width=plane.width, annotate_grids=True,
                      output=str(tmp_path / "s.png"))
    assert np.isfinite(image).sum() > 1000
    after = frames()
    assert (before[0] != 0).sum() > 500 and before[3].any()
    assert np.array_equal(bits(before[0]), bits(after[0]))
    assert np.array_equal(before[1], after[1])
    assert np.array_equal(before[2].view(np.uint32), after[2].view(np.uint32))
    assert np.array_equal(before[3], after[3])
