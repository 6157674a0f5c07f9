"""Off-axis projections without a GPU: rays.pixel_rays and rays.pixel_order against a literal loop;
the image layer (api.project_off_axis_scene with the device call answered by ray_sums_reference)
against things that are not the walk -- the covering grid's finest columns and the on-axis
projection's reference for an axis view, an analytic slab intersection for a constant field along
a generic direction, the mirror image for the reversed normal; the host side of
api.project_off_axis with the device work patched out; and the declared ABI entry."""
import math
import os
import types

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, plotfile
from amrvolumerenderer_amd import rays as ray_rules

import axis_projection_reference as axis_ref
import covering_grid_reference as grid_ref
import gradient_reference as ref
import ray_reference as rr
import ray_sums_reference as sums_ref
from test_rays import AXIS_CASES, AXIS_HI, AXIS_LO, THREE_BOXES, THREE_DOMAINS, THREE_HI, THREE_LO, Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_LAYER, SUMS_LAYER = api.project_off_axis_scene, api.ray_sums_scene    # before any patch
EPS = 2.0 ** -52
GENERIC = (1.0, 0.7, 0.4)


# ---- rays.py ---------------------------------------------------------------------------------------

SIZES = [(1, 1), (8, 8), (9, 7), (64, 1), (17, 16)]


@pytest.mark.parametrize("width,height", SIZES)
def test_pixel_order_lists_every_pixel_once_tile_by_tile(width, height):
    order = ray_rules.pixel_order(width, height)
    assert order.dtype == np.int64 and sorted(order.tolist()) == list(range(width * height))
    want = []
    for ty in range((height + 7) // 8):
        for tx in range((width + 7) // 8):
            for py in range(8):
                for px in range(8):
                    x, y = 8 * tx + px, 8 * ty + py
                    if x < width and y < height:
                        want.append(y * width + x)
    assert order.tolist() == want
    if width % 8 == 0 and height % 8 == 0:
        # a wave's 64 rays are one tile
        for first in range(0, width * height, 64):
            y, x = np.divmod(order[first:first + 64], width)
            assert x.max() - x.min() == 7 and y.max() - y.min() == 7


def test_pixel_order_and_pixel_rays_refuse_an_empty_image():
    for wrong in ((0, 4), (4, 0), (-1, 4)):
        with pytest.raises(ValueError):
            ray_rules.pixel_order(*wrong)
        with pytest.raises(ValueError):
            ray_rules.pixel_rays((0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 1, 0), (1, 1), 1, *wrong)


@pytest.mark.parametrize("width,height", SIZES)
def test_pixel_rays_against_a_loop_over_the_pixels(width, height):
    center, widths, depth = (0.3, -1.7, 2.9), (2.3, 1.1), 5.7
    n, U, V = api.slice_basis(GENERIC, (0.1, 0.2, 1.0))
    start, end = ray_rules.pixel_rays(center, n, U, V, widths, depth, width, height)
    assert start.shape == end.shape == (height * width, 3) and start.dtype == np.float64
    h = 0.5 * depth
    for y in range(height):
        for x in range(width):
            su = ((x + 0.5) / width - 0.5) * widths[0]
            sv = ((y + 0.5) / height - 0.5) * widths[1]
            P = [(center[d] + su * U[d]) + sv * V[d] for d in range(3)]
            assert start[y * width + x].tolist() == [P[d] + h * n[d] for d in range(3)]
            assert end[y * width + x].tolist() == [P[d] - h * n[d] for d in range(3)]
    # with n pointing at the viewer the rays run away from the viewer
    assert (((end - start) @ np.array(n)) < 0.0).all()


# ---- the image layer over the reference ----------------------------------------------------------

def _scene(name):
    """A scene the patched ray_sums_scene tells apart by its name."""
    return types.SimpleNamespace(name=name, local_boxes=[0], all_boxes=[0])


def _reference_images(monkeypatch, case, component, weight, center, normal, north, plane_width,
                      depth, width, height, min_level=0, max_level=-1):
    """api.project_off_axis_scene with ray_sums_scene answered by ray_sums_reference: the image
    layer as it runs, the kernel replaced by the reference.  Also returns, per pixel in row-major
    order, sum |v w| over the counted segments."""
    seen = {}

    def fake(ctx, scene, start, end, cell_sizes, prob_lo, ref_ratio, weight_scene=None,
             max_trips=None, rank=0, n_ranks=1):
        assert scene.name == "field" and (weight_scene is None) == (weight is None)
        field = case.hierarchy(component, min_level, max_level)
        other = None if weight is None else case.hierarchy(weight, min_level, max_level)
        walk = field.rays(start, end, field.default_max_trips())
        seen["start"], seen["walk"] = start, walk
        return sums_ref.sums_of(start, end, walk,
                                None if other is None else other.rays(start, end,
                                                                      other.default_max_trips()))

    monkeypatch.setattr(api, "ray_sums_scene", fake)
    images = api.project_off_axis_scene(
        "ctx", _scene("field"), None if weight is None else _scene("weight"), center, normal, north,
        plane_width, depth, width, height, case.sizes, case.lo, case.ratio, tile_order=True)
    # the rays went out tile by tile
    start, _ = ray_rules.pixel_rays(center, *api.slice_basis(normal, north), plane_width, depth,
                                    width, height)
    order = ray_rules.pixel_order(width, height)
    assert seen["start"].tobytes() == start[order].tobytes()
    return images


@pytest.mark.parametrize("ratios", ["2-2", "2-4"])
def test_an_axis_view_gives_the_covering_grids_columns_and_the_on_axis_projection(monkeypatch, ratios):
    """normal z, north y: U = x and V = y, so with the finest level's (nx, ny) pixels over the
    domain every ray runs through the centres of a finest-level column.  Extents and cell sizes
    are powers of two: every T is exact."""
    ratio, domains, boxes, _ = AXIS_CASES[ratios]
    case = Case(domains, boxes, AXIS_LO, AXIS_HI, ratio, 82)
    nx, ny, nz = (domains[2][1][d] + 1 for d in range(3))
    center, widths, depth = (1.0, 0.5, 0.5), (2.0, 1.0), 2.0
    view = ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0))
    assert api.slice_basis(*view) == ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    dz = case.sizes[2][2]
    grids = [grid_ref.covering_grid(case.levels, case.ratio, c, 2, [0, 0, 0], [nx, ny, nz])
             for c in (0, 2)]
    u, whole = (g["values"].reshape(nz, ny, nx) for g in grids)
    assert np.isfinite(u).all() and np.isfinite(whole).all()
    for weight in (None, 2):
        got = _reference_images(monkeypatch, case, 0, weight, center, *view, widths, depth, nx, ny)
        assert (got["status"] == rr.COMPLETE).all() and (got["covered"] == 1.0).all()
        assert (got["counted"] == 1.0).all() and got["count"].min() >= 4
        terms = (u if weight is None else u * whole) * dz          # dz: a power of two
        count = got["count"].astype(np.float64)
        worst = 0.0
        for y in range(ny):
            for x in range(nx):
                column = math.fsum(terms[:, y, x].tolist())
                bound = count[y, x] * EPS * math.fsum(np.abs(terms[:, y, x]).tolist())
                assert abs(got["integral"][y, x] - column) <= bound, (x, y)
                worst = max(worst, abs(got["integral"][y, x] - column) / bound)
                if weight is not None:
                    below = (whole[:, y, x] * dz).tolist()
                    assert abs(got["weight"][y, x] - math.fsum(below)) <= \
                        count[y, x] * EPS * math.fsum(abs(t) for t in below), (x, y)
        print("weight:", weight, "worst error / bound:", worst)
        if ratio != [2, 2]:
            continue
        # the on-axis projection's reference, which knows ratio 2 only: the integral and, for the
        # weighted mean, its numerator and its denominator
        want = axis_ref.reference(case.levels, AXIS_LO, AXIS_HI, 2, 0, weight, center, widths, nx,
                                  ny, [size[2] for size in case.sizes], with_fsum=True)
        assert np.array_equal(want["count"], got["count"])
        assert (np.abs(got["integral"] - want["integral_fsum"]) <=
                count * EPS * want["integral_abs"]).all()
        if weight is not None:
            assert (np.abs(got["weight"] - want["weight_fsum"]) <=
                    count * EPS * want["weight_abs"]).all()


def _constant(value):
    case = Case(THREE_DOMAINS, THREE_BOXES, THREE_LO, THREE_HI, [2, 2], 84)
    for level in case.levels:
        for cells in level["data"]:
            cells[...] = value
    return case


def _whole_view(case):
    lo, hi = np.array(case.lo), np.array(case.hi)
    diagonal = float(np.sqrt(((hi - lo) ** 2).sum()))
    return tuple(0.5 * (lo + hi)), (diagonal, diagonal), diagonal


def test_a_constant_field_gives_the_chord_through_the_domain_box(monkeypatch):
    c = 3.0
    case = _constant(c)
    center, widths, depth = _whole_view(case)
    width, height = 16, 8
    got = _reference_images(monkeypatch, case, 0, None, center, GENERIC, (0.0, 0.0, 1.0), widths,
                            depth, width, height)
    # the slab intersection of every pixel's segment with the box [lo, hi]
    start, end = ray_rules.pixel_rays(center, *api.slice_basis(GENERIC, (0.0, 0.0, 1.0)), widths,
                                      depth, width, height)
    d = end - start
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    assert (d != 0.0).all()
    near = (np.where(d > 0.0, case.lo, case.hi) - start) / d
    far = (np.where(d > 0.0, case.hi, case.lo) - start) / d
    t0, t1 = np.maximum(near.max(axis=1), 0.0), np.minimum(far.min(axis=1), 1.0)
    hit = (t0 < t1).reshape(height, width)
    chord = np.where(hit, ((t1 - t0) * length).reshape(height, width), 0.0)
    assert 40 < hit.sum() < width * height
    assert np.array_equal(got["status"] == rr.COMPLETE, hit)
    assert np.array_equal(got["status"] == rr.MISS, ~hit)
    bound = got["count"] * EPS * chord
    print("worst error / bound:", (np.abs(got["covered"] - chord)[hit] / bound[hit]).max(),
          (np.abs(got["integral"] - c * chord)[hit] / (c * bound[hit])).max())
    assert (np.abs(got["covered"] - chord) <= bound).all()
    assert (np.abs(got["integral"] - c * chord) <= c * bound).all()
    assert ref.same_bits(got["counted"], got["covered"])
    # pixels that miss: nothing counted, and a mean that is NaN
    assert (got["counted"][~hit] == 0.0).all() and (got["count"][~hit] == 0).all()
    with np.errstate(all="ignore"):
        mean = np.where(got["counted"] != 0.0, got["integral"] / got["counted"], math.nan)
    assert np.isnan(mean[~hit]).all() and (np.abs(mean[hit] - c) <= 4 * EPS * c * 64).all()


def test_the_reversed_normal_gives_the_mirror_image(monkeypatch):
    """-normal with the same north: U flips and V stays, and with a width that is a power of two
    pixel (x, y) owns the reversed ray of pixel (W - 1 - x, y).  The two walks round other
    parameters (t against 1 - t), so a segment's length differs by up to 2^-53 |D| between them,
    whatever its own size: against a bound that is relative to sum |v w|, over the part of the ray
    inside the data, that only holds for rays whose chord is comparable to their length.  So the
    view is the middle of the domain -- half its shortest edge wide, every chord above a third of
    |D| -- not its corners, where a ray of the same length clips a chord a hundred times shorter."""
    case = Case(THREE_DOMAINS, THREE_BOXES, THREE_LO, THREE_HI, [2, 2], 81)
    center, _, depth = _whole_view(case)
    widths = (0.5, 0.5)
    width, height = 16, 8
    north = (0.0, 0.0, 1.0)
    back = tuple(-v for v in GENERIC)
    ahead_rays = ray_rules.pixel_rays(center, *api.slice_basis(GENERIC, north), widths, depth, width,
                                      height)
    back_rays = ray_rules.pixel_rays(center, *api.slice_basis(back, north), widths, depth, width,
                                     height)
    mirror = lambda a: a.reshape(height, width, -1)[:, ::-1].reshape(a.shape)
    assert ahead_rays[0].tobytes() == mirror(back_rays[1]).tobytes()
    assert ahead_rays[1].tobytes() == mirror(back_rays[0]).tobytes()
    ahead = _reference_images(monkeypatch, case, 0, None, center, GENERIC, north, widths, depth,
                              width, height)
    behind = _reference_images(monkeypatch, case, 0, None, center, back, north, widths, depth,
                               width, height)
    # sum |v w| of every ray, from the segments
    hierarchy = case.hierarchy()
    walk = hierarchy.rays(*ahead_rays, hierarchy.default_max_trips())
    d = ahead_rays[1] - ahead_rays[0]
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    magnitude = np.array([
        math.fsum((np.abs(walk["value"][a:b]) * (walk["t1"][a:b] - walk["t0"][a:b]) * length[s]).tolist())
        for s, (a, b) in enumerate(zip(walk["offsets"][:-1], walk["offsets"][1:]))])
    magnitude = magnitude.reshape(height, width)
    assert np.array_equal(ahead["status"], behind["status"][:, ::-1])
    assert (ahead["status"] == rr.COMPLETE).all()
    assert (ahead["covered"] > length.reshape(height, width) / 3.0).all()
    count = np.maximum(ahead["count"], behind["count"][:, ::-1]).astype(np.float64)
    error = np.abs(ahead["integral"] - behind["integral"][:, ::-1])
    walked = ahead["status"] == rr.COMPLETE
    print("worst error / bound:", (error[walked] / (count * EPS * magnitude)[walked]).max())
    assert (error <= count * EPS * magnitude).all()
    assert (ahead["integral"] != behind["integral"][:, ::-1]).any()     # not the same sums again


# ---- the host layer with the device work patched out ---------------------------------------------

def _tiny_plotfile(path):
    levels = ref.make_levels([((0, 0, 0), (3, 3, 3)), ((0, 0, 0), (7, 7, 7))],
                             [[((0, 0, 0), (3, 3, 3))], [((2, 2, 2), (5, 5, 5))]], [2], 53)
    plotfile.write_plotfile(str(path), list(ref.VARIABLES), levels, (0.0, -1.0, 2.0),
                            (1.0, 1.0, 6.0), [2])
    return str(path)


def _patched(monkeypatch, world=1, local=2, status=None, weight_zero=()):
    """api.project_off_axis without a device: _load_fields answers with scenes of two boxes that
    span (0, -1, 2) .. (1, 1, 6) at a world scale of 2, project_off_axis_scene with images made
    from the pixel numbers."""
    asked = []
    box = lambda lo, hi: types.SimpleNamespace(min_corner=tuple(2.0 * v for v in lo),
                                               max_corner=tuple(2.0 * v for v in hi), level=0)
    boxes = [box((0.0, -1.0, 2.0), (0.5, 1.0, 6.0)), box((0.5, -1.0, 2.0), (1.0, 1.0, 6.0))]

    def fake_load_fields(path, variables, min_level, max_level):
        asked.append(("load", tuple(variables), min_level, max_level))
        scenes = [types.SimpleNamespace(name=name, all_boxes=boxes, local_boxes=boxes[:local],
                                        world_scale=2.0) for name in variables]
        return "ctx", 0, world, None, scenes, [0.125, 0.015625]

    def fake_scene(ctx, scene_f, scene_w, center, normal, north, plane_width, depth, width, height,
                   cell_sizes, prob_lo, ref_ratio, rank=0, n_ranks=1):
        assert ctx == "ctx" and len(cell_sizes) == 2 and list(ref_ratio) == [2]
        assert list(prob_lo) == [0.0, -1.0, 2.0] and (rank, n_ranks) == (0, world)
        asked.append((scene_f.name, None if scene_w is None else scene_w.name, center, normal,
                      north, plane_width, depth, width, height))
        pixel = np.arange(width * height, dtype=np.float64).reshape(height, width)
        counted = np.where(pixel % 5 == 0, 0.0, 2.0)
        below = pixel + 1.0
        for at in weight_zero:
            below[at] = 0.0
        state = np.zeros((height, width), dtype=np.uint8)
        if status is not None:
            state[status[0]] = status[1]
        return {"integral": 3.0 * pixel, "weight": None if scene_w is None else below,
                "counted": counted, "covered": np.full((height, width), 2.0), "status": state,
                "count": np.full((height, width), 4, dtype=np.uint32)}

    monkeypatch.setattr(api, "_load_fields", fake_load_fields)
    monkeypatch.setattr(api, "project_off_axis_scene", fake_scene)
    return asked


def test_project_off_axis_fills_in_the_defaults_and_forms_the_quantities(tmp_path, monkeypatch):
    path = _tiny_plotfile(tmp_path / "plt")
    asked = _patched(monkeypatch, weight_zero=[(1, 2)])
    column = api.project_off_axis(path, GENERIC, variable="u", width=4, height=3, min_level=1)
    diagonal = math.sqrt((1.0 * 1.0 + 2.0 * 2.0) + 4.0 * 4.0)
    assert asked == [("load", ("u",), 1, -1),
                     ("u", None, (0.5, 0.0, 4.0), GENERIC, (0.0, 0.0, 1.0), (diagonal, diagonal),
                      diagonal, 4, 3)]
    pixel = np.arange(12, dtype=np.float64).reshape(3, 4)
    assert column.dtype == np.float64 and ref.same_bits(column, 3.0 * pixel)
    # a mean: integral / counted, NaN where nothing was counted
    mean = api.project_off_axis(path, GENERIC, width=4, height=3, quantity="mean")
    assert asked[-2] == ("load", ("",), 0, -1) and asked[-1][0] == ""
    assert np.isnan(mean[pixel % 5 == 0]).all() and np.isnan(mean).sum() == 3
    assert ref.same_bits(mean[pixel % 5 != 0], (3.0 * pixel / 2.0)[pixel % 5 != 0])
    # a weight: integral / weight, NaN where the weight's sum is 0, whatever was counted
    weighted = api.project_off_axis(path, GENERIC, variable="u", weight="whole", width=4, height=3,
                                    quantity="mean")
    assert asked[-2] == ("load", ("u", "whole"), 0, -1) and asked[-1][:2] == ("u", "whole")
    assert np.isnan(weighted[1, 2]) and np.isnan(weighted).sum() == 1
    keep = np.isfinite(weighted)
    assert ref.same_bits(weighted[keep], (3.0 * pixel / (pixel + 1.0))[keep])
    # what is given is passed on; along +-z north defaults to y
    api.project_off_axis(path, (0.0, 0.0, -2.0), width=4, height=3, center=(1, 2, 3),
                         plane_width=(4, 5), depth=6)
    assert asked[-1][2:] == ((1.0, 2.0, 3.0), (0.0, 0.0, -2.0), (0.0, 1.0, 0.0), (4.0, 5.0), 6.0, 4, 3)
    api.project_off_axis(path, (1e-7, 0.0, 1.0), width=4, height=3)
    assert asked[-1][4] == (0.0, 1.0, 0.0)
    api.project_off_axis(path, (1e-5, 0.0, 1.0), width=4, height=3)
    assert asked[-1][4] == (0.0, 0.0, 1.0)
    api.project_off_axis(path, (0.0, 0.0, 1.0), width=4, height=3, north=(1.0, 0.0, 0.0))
    assert asked[-1][4] == (1.0, 0.0, 0.0)


def test_project_off_axis_refuses_wrong_arguments_before_the_plotfile_is_opened(monkeypatch):
    def never(*arguments, **named):
        raise AssertionError("the plotfile was opened")

    monkeypatch.setattr(api, "_load_fields", never)
    monkeypatch.setattr(api, "_require_plotfile", never)
    ok = dict(normal=GENERIC, width=4, height=3)
    wrong = [
        (dict(width=0), "image dimensions must be positive"),
        (dict(height=-1), "image dimensions must be positive"),
        (dict(quantity="max"), "quantity must be one of column, mean, not 'max'"),
        (dict(center=(0.0, 1.0)), "center must hold three finite values"),
        (dict(center=(0.0, math.nan, 1.0)), "center must hold three finite values"),
        (dict(plane_width=(1.0,)), "plane_width must hold two values (wu, wv)"),
        (dict(plane_width=(1.0, 0.0)), "plane_width must be finite and positive"),
        (dict(depth=0.0), "depth must be finite and positive"),
        (dict(depth=math.inf), "depth must be finite and positive"),
        (dict(normal=(0.0, 0.0)), "normal must hold three values"),
        (dict(normal=(0.0, 0.0, 0.0)), "normal must be a finite, non-zero vector"),
        (dict(normal=(0.0, math.inf, 0.0)), "normal must be a finite, non-zero vector"),
        (dict(north=(0.0, 0.0, 0.0)), "north must be a finite, non-zero vector"),
        (dict(north=GENERIC), "north must not be parallel to the normal"),
        (dict(value_range=(1.0,)), "value_range must hold two values (lo, hi)"),
        (dict(value_range=(2.0, 1.0)), "value_range must satisfy lo < hi"),
        (dict(value_range=(0.0, 1.0), log_scale=True),
         "value_range must be positive when log_scale is enabled"),
        (dict(weight=""), "weight must be a variable name or None, not ''"),
        (dict(weight=3), "weight must be a variable name or None, not 3"),
        (dict(weight="whole"), 'a weighted projection is a mean: quantity="column" takes no weight'),
    ]
    for arguments, text in wrong:
        with pytest.raises(ValueError) as caught:
            api.project_off_axis("plt", **{**ok, **arguments})
        assert str(caught.value) == text, arguments
    with pytest.raises(ValueError, match="color_map entries"):
        api.project_off_axis("plt", **ok, color_map=[(0.0, 1.0, 1.0)])
    # the validator returns what the call goes on with
    assert api.validate_off_axis_projection_arguments(4, 3, (0, 0, 2), "mean", (1, 2, 3), (4, 5), 6,
                                                      None, False, (1, 2), "w") == \
        ((0.0, 0.0, 2.0), (0.0, 1.0, 0.0), (1.0, 2.0, 3.0), (4.0, 5.0), 6.0, (1.0, 2.0))
    assert api.validate_off_axis_projection_arguments(4, 3, GENERIC) == \
        (GENERIC, (0.0, 0.0, 1.0), None, None, None, None)


def test_a_truncated_ray_is_an_error_that_names_the_pixel(tmp_path, monkeypatch):
    path = _tiny_plotfile(tmp_path / "plt")
    _patched(monkeypatch, status=((2, 1), rr.TRUNCATED))
    with pytest.raises(RuntimeError, match=r"pixel \(x=1, y=2\)"):
        api.project_off_axis(path, GENERIC, width=4, height=3)
    _patched(monkeypatch, status=((2, 1), rr.MISS))                   # a miss is no error
    assert api.project_off_axis(path, GENERIC, width=4, height=3).shape == (3, 4)


def test_several_ranks_are_not_implemented(tmp_path, monkeypatch):
    path = _tiny_plotfile(tmp_path / "plt")
    asked = _patched(monkeypatch, world=2)
    with pytest.raises(NotImplementedError, match="on one rank"):
        api.project_off_axis(path, GENERIC, width=4, height=3)
    assert asked == [("load", ("",), 0, -1)]                          # no projection was started
    asked = _patched(monkeypatch, local=1)                            # a box on another rank
    with pytest.raises(NotImplementedError):
        api.project_off_axis(path, GENERIC, width=4, height=3)
    assert len(asked) == 1
    # a launcher's world size is known before anything is loaded
    asked = _patched(monkeypatch)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(NotImplementedError):
        api.project_off_axis(path, GENERIC, width=4, height=3)
    assert asked == []

    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"the context was used ({name})")

    part = types.SimpleNamespace(local_boxes=[0], all_boxes=[0, 1])
    whole = types.SimpleNamespace(local_boxes=[0], all_boxes=[0])
    view = ((0.5, 0.5, 0.5), GENERIC, (0.0, 0.0, 1.0), (1.0, 1.0), 2.0, 4, 3, [(0.25,) * 3],
            (0.0, 0.0, 0.0), [])
    with pytest.raises(NotImplementedError):
        SCENE_LAYER(NoDevice(), part, None, *view)
    with pytest.raises(NotImplementedError):
        SCENE_LAYER(NoDevice(), whole, None, *view, rank=0, n_ranks=2)
    with pytest.raises(NotImplementedError):
        SUMS_LAYER(NoDevice(), part, [[0.0, 0.0, 0.0]], [[1.0, 1.0, 1.0]], *view[7:])


def test_the_image_layer_undoes_the_tile_order(monkeypatch):
    """A device answer made from every ray's own end points comes back at the ray's pixel."""
    width, height = 9, 7
    center, widths, depth = (0.5, 0.25, -1.0), (2.0, 3.0), 4.0

    def fake(ctx, scene, start, end, cell_sizes, prob_lo, ref_ratio, weight_scene=None,
             max_trips=None, rank=0, n_ranks=1):
        assert max_trips is None and weight_scene.name == "weight"
        n = start.shape[0]
        return {"count": (np.arange(n) % 7).astype(np.uint32),
                "status": (start[:, 0] > 0.5).astype(np.uint8), "t_enter": np.zeros(n),
                "t_leave": np.ones(n), "integral": start[:, 0] + 2.0 * start[:, 1],
                "weight": end[:, 2], "counted": end[:, 0], "covered": start[:, 2]}

    monkeypatch.setattr(api, "ray_sums_scene", fake)
    got = api.project_off_axis_scene("ctx", _scene("field"), _scene("weight"), center, GENERIC,
                                     (0.0, 0.0, 1.0), widths, depth, width, height, [(1.0,) * 3],
                                     (0.0, 0.0, 0.0), [], tile_order=True)
    start, end = ray_rules.pixel_rays(center, *api.slice_basis(GENERIC, (0.0, 0.0, 1.0)), widths,
                                      depth, width, height)
    image = lambda a: a.reshape(height, width)
    assert ref.same_bits(got["integral"], image(start[:, 0] + 2.0 * start[:, 1]))
    assert ref.same_bits(got["weight"], image(end[:, 2]))
    assert ref.same_bits(got["counted"], image(end[:, 0]))
    assert ref.same_bits(got["covered"], image(start[:, 2]))
    assert np.array_equal(got["status"], image((start[:, 0] > 0.5).astype(np.uint8)))
    assert got["status"].dtype == np.uint8 and got["count"].dtype == np.uint32
    order = ray_rules.pixel_order(width, height)
    count = np.empty(width * height, dtype=np.uint32)
    count[order] = np.arange(width * height) % 7
    assert np.array_equal(got["count"], image(count))
    # by default the rays go out in row-major order, and the images are the same
    plain = api.project_off_axis_scene("ctx", _scene("field"), _scene("weight"), center, GENERIC,
                                       (0.0, 0.0, 1.0), widths, depth, width, height, [(1.0,) * 3],
                                       (0.0, 0.0, 0.0), [])
    assert np.array_equal(plain["count"], image(np.arange(width * height) % 7))
    assert all(plain[key].tobytes() == got[key].tobytes() for key in got if key != "count")
    for wrong in (dict(width=0), dict(depth=0.0), dict(plane_width=(1.0, -1.0)),
                  dict(center=(0.0, 0.0, math.inf))):
        named = dict(center=center, plane_width=widths, depth=depth, width=width, height=height)
        named.update(wrong)
        with pytest.raises(ValueError):
            api.project_off_axis_scene("ctx", _scene("field"), _scene("weight"), named["center"],
                                       GENERIC, (0.0, 0.0, 1.0), named["plane_width"],
                                       named["depth"], named["width"], named["height"],
                                       [(1.0,) * 3], (0.0, 0.0, 0.0), [])


# ---- the ABI entry ---------------------------------------------------------------------------------

def test_the_entry_is_declared_with_19_arguments_and_the_rays_keep_22(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    declared = header[header.index("int avr_scene_ray_sums("):]
    declared = declared[:declared.index(";")]
    assert declared.count(",") + 1 == 19
    assert "int avr_scene_ray_sums(avr_context *ctx, const avr_scene *field, const avr_scene *weight" \
        in header
    assert len(_capi.SIGNATURES["avr_scene_ray_sums"][1]) == 19
    assert len(_capi.SIGNATURES["avr_scene_rays"][1]) == 22
    assert getattr(avr_lib, "avr_scene_ray_sums") is not None
    assert getattr(avr_lib, "avr_scene_rays") is not None
    assert avr_lib.avr_abi_version() == 2
