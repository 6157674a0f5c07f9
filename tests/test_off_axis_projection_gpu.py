"""Per-ray sums and off-axis projections on the GPU: the sums mode of avr_rays.hip through
avr_scene_ray_sums, api.ray_sums_scene, api.project_off_axis_scene and api.project_off_axis.
Everything is compared by bits: with the count and the emit pass of avr_scene_rays on the same
scene, and with ray_sums_reference, which sums the segments that ray_reference lists.  The
hierarchies are test_rays_gpu's: cell sizes are powers of two and every covered coarse cell holds
1e30."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api
from amrvolumerenderer_amd import rays as ray_rules

import derive_reference
import gradient_reference as ref
import ray_reference as rr
import ray_sums_reference as sums_ref
import test_rays_gpu as base

pytestmark = pytest.mark.gpu
VARIABLES = list(ref.VARIABLES)
SUMS = ("integral", "weight", "counted", "covered")


@pytest.fixture(autouse=True)
def _empty_registries():
    def clear():
        for name in list(api.derived_fields()):
            api.remove_field(name)
    clear()
    yield
    clear()


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    return base._write(tmp_path_factory.mktemp("sums") / "three", base.THREE_DOMAINS,
                       base.THREE_BOXES, (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 2], 91)


@pytest.fixture(scope="module")
def two_four(tmp_path_factory):
    """The same grids under ratios 2 and 4."""
    domains = [((0, 0, 0), (11, 5, 7)), ((0, 0, 0), (23, 11, 15)), ((0, 0, 0), (95, 47, 63))]
    boxes = [base.THREE_BOXES[0], base.THREE_BOXES[1], [((24, 12, 12), (43, 27, 31))]]
    return base._write(tmp_path_factory.mktemp("sums") / "two_four", domains, boxes,
                       (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 4], 95)


def wanted(case, start, end, name, weight=None, max_trips=None, min_level=0, max_level=-1):
    """The reference's sums of `name` (weighted by `weight`) along start -> end."""
    field = case.reference(name, min_level, max_level)
    other = None if weight is None else case.reference(weight, min_level, max_level)
    return sums_ref.ray_sums(start, end, field, other, max_trips)


def same_sums(got, want, weighted):
    print("rays:", want["count"].size, "segments:", int(want["count"].sum()), "status:",
          np.bincount(got["status"], minlength=4).tolist(), "reference:",
          np.bincount(want["status"], minlength=4).tolist())
    assert got["count"].dtype == np.uint32 and np.array_equal(got["count"], want["count"])
    assert got["status"].dtype == np.uint8 and np.array_equal(got["status"], want["status"])
    assert (got["weight"] is not None) == weighted == (want["weight"] is not None)
    for key in ("t_enter", "t_leave") + SUMS:
        if got[key] is not None:
            assert got[key].dtype == np.float64 and ref.same_bits(got[key], want[key]), key


def scene_sums(ctx, case, name, weight, n, max_trips=None, min_level=0, max_level=-1):
    scene = base.load(ctx, case, name, min_level, max_level)
    other = None if weight is None else base.load(ctx, case, weight, min_level, max_level)
    finest = max(b.level for b in scene.all_boxes)
    start, end = case.rays(n)
    got = api.ray_sums_scene(ctx, scene, start, end, case.sizes()[:finest + 1], case.lo,
                             case.ratio[:finest], other, max_trips)
    want = wanted(case, start, end, name, weight, max_trips, min_level, max_level)
    same_sums(got, want, weight is not None)
    return got, want


# ---- the ABI entry, beside the two existing passes ------------------------------------------------

class Buffers:
    """The seven outputs, filled with sentinels."""

    def __init__(self, device, n):
        self.counts = torch.full((n,), -7, dtype=torch.int32, device=device)
        self.status = torch.full((n,), 9, dtype=torch.uint8, device=device)
        self.span = torch.full((n, 2), 0.5, dtype=torch.float64, device=device)
        self.integral, self.weight, self.counted, self.covered = (
            torch.full((n,), 0.125, dtype=torch.float64, device=device) for _ in range(4))

    def untouched(self):
        return bool((self.counts == -7).all()) and bool((self.status == 9).all()) and \
            bool((self.span == 0.5).all()) and all(
                bool((t == 0.125).all())
                for t in (self.integral, self.weight, self.counted, self.covered))

    def result(self, weighted):
        host = lambda t: t.cpu().numpy()
        span = host(self.span)
        return {"count": host(self.counts).view(np.uint32), "status": host(self.status),
                "t_enter": span[:, 0].copy(), "t_leave": span[:, 1].copy(),
                "integral": host(self.integral), "weight": host(self.weight) if weighted else None,
                "counted": host(self.counted), "covered": host(self.covered)}


def pointer(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def call_sums(ctx, case, field, weight, start, end, out, n_rays=None, max_trips=None, index=None,
              n_levels=None, **replaced):
    """avr_scene_ray_sums itself; replaced: output arrays by their argument's name."""
    n_levels = len(case.levels) if n_levels is None else n_levels
    index = np.ascontiguousarray([lo for _, lo, _ in case.scene_boxes()] if index is None
                                 else index, np.int32)
    ratio = np.ascontiguousarray(case.ratio, np.int32)
    sizes = np.ascontiguousarray(case.sizes(), np.float64)
    prob_lo = np.ascontiguousarray(case.lo, np.float64)
    arrays = dict(counts=out.counts, status=out.status, span=out.span, integral=out.integral,
                  weight_out=out.weight if weight is not None else None, counted=out.counted,
                  covered=out.covered, start=start, end=end)
    arrays.update(replaced)
    torch.cuda.synchronize()      # the fills of torch's stream are done before the context's runs
    return _capi.lib().avr_scene_ray_sums(
        ctx._handle, field._handle, weight._handle if weight is not None else None,
        pointer(arrays["start"]), pointer(arrays["end"]),
        int(start.shape[0]) if n_rays is None else n_rays,
        case.reference("u").default_max_trips() if max_trips is None else max_trips,
        index.ctypes.data_as(C.POINTER(C.c_int32)), ratio.ctypes.data_as(C.POINTER(C.c_int32)),
        sizes.ctypes.data_as(C.POINTER(C.c_double)), prob_lo.ctypes.data_as(C.POINTER(C.c_double)),
        n_levels, pointer(arrays["counts"]), pointer(arrays["status"]), pointer(arrays["span"]),
        pointer(arrays["integral"]), pointer(arrays["weight_out"]), pointer(arrays["counted"]),
        pointer(arrays["covered"]))


@pytest.mark.parametrize("which", ["three", "two_four"])
def test_the_pool_gives_the_count_pass_the_emit_pass_and_the_reference(ctx, request, which):
    case = request.getfixturevalue(which)
    u = base.load(ctx, case, "u")
    su = ctx.create_scene(u.local_boxes, u.scalar_transform)
    n = 256
    start_host, end_host = case.rays(n)
    start = torch.from_numpy(start_host).to(ctx.device)
    end = torch.from_numpy(end_host).to(ctx.device)
    out = Buffers(ctx.device, n)
    assert call_sums(ctx, case, su, None, start, end, out) == 0, _capi.lib().avr_last_error()
    ctx.synchronize()
    assert bool((out.weight == 0.125).all())            # no weight: its array is not looked at
    got = out.result(False)
    # the two existing passes on the same scene, on the device
    index = np.array([lo for _, lo, _ in case.scene_boxes()], dtype=np.int32)
    arguments = (start, end, case.reference("u").default_max_trips(), index, case.ratio,
                 case.sizes(), case.lo)
    counts, status, span = su.rays(*arguments)
    offsets = torch.zeros(n + 1, dtype=torch.int64, device=ctx.device)
    torch.cumsum(counts.to(torch.int64), 0, out=offsets[1:])
    ctx.synchronize()
    *_, integral, covered = su.rays(*arguments, offsets=offsets, n_segments=int(offsets[-1].item()))
    ctx.synchronize()
    assert np.array_equal(got["count"], counts.cpu().numpy().view(np.uint32))
    assert np.array_equal(got["status"], status.cpu().numpy())
    assert ref.same_bits(got["t_enter"], span.cpu().numpy()[:, 0])
    assert ref.same_bits(got["t_leave"], span.cpu().numpy()[:, 1])
    assert ref.same_bits(got["integral"], integral.cpu().numpy())
    assert ref.same_bits(got["covered"], covered.cpu().numpy())
    same_sums(got, wanted(case, start_host, end_host, "u"), False)
    assert got["status"][:6].tolist() == [0, 1, 1, 3, 3, 3] and (got["status"] == 0).sum() > 150
    assert got["count"].sum() > 2000 and (got["status"] == 2).sum() == 0
    # without a hole and without a value that is not finite, all of a ray's length is counted
    assert ref.same_bits(got["counted"], got["covered"])
    su.close()


# ---- a weight field ---------------------------------------------------------------------------------

def test_a_stored_field_as_the_weight(ctx, three):
    got, _ = scene_sums(ctx, three, "u", "whole", 256)
    assert ref.same_bits(got["counted"], got["covered"]) and np.abs(got["weight"]).max() > 10.0


@pytest.mark.parametrize("field,weight", [("odd", "u"), ("u", "odd"), ("odd", "odd"), ("odd", None)])
def test_only_cells_where_both_are_finite_count(ctx, three, field, weight):
    got, _ = scene_sums(ctx, three, field, weight, 256)
    assert all(np.isfinite(got[key]).all() for key in SUMS if got[key] is not None)
    walked = got["status"] == 0
    assert (got["counted"] <= got["covered"])[walked].all()
    assert (got["counted"] < got["covered"]).sum() > 5


def test_a_derived_field_as_the_weight_is_another_allocation(three):
    api.add_field("uu", "u * u + 1.0")
    own, rank, world, _, scenes, _ = api._load_fields(three.path, ["u", "uu"], 0, -1)
    cells = lambda scene: {int(b.values.untyped_storage().data_ptr()) for b in scene.local_boxes}
    assert len(cells(scenes[1])) == 1 and not cells(scenes[1]) & cells(scenes[0])
    start, end = three.rays(256)
    got = api.ray_sums_scene(own, scenes[0], start, end, three.sizes(), three.lo, three.ratio,
                             scenes[1], None, rank, world)
    squared = derive_reference.evaluate_levels("u * u + 1.0", three.levels, VARIABLES, three.lo,
                                               three.hi)
    levels = [{"domain": lev["domain"], "boxes": lev["boxes"], "data": [g[None] for g in grids]}
              for lev, grids in zip(three.levels, squared)]
    weight = rr.Hierarchy(levels, three.ratio, 0, three.sizes(), three.lo)
    same_sums(got, sums_ref.ray_sums(start, end, three.reference("u"), weight), True)
    assert (got["weight"][got["status"] == 0] > 0.0).all()


# ---- sizes, truncation, holes -------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_the_last_waves_bounds(ctx, three, n):
    scene_sums(ctx, three, "whole", "u", n)


def test_max_trips_truncates_with_the_partial_sums(ctx, three):
    got, _ = scene_sums(ctx, three, "u", "whole", 256, 3)
    assert (got["status"] == 2).sum() > 150 and got["count"].max() <= 3
    assert (got["covered"][got["status"] == 2] > 0.0).any()
    got, _ = scene_sums(ctx, three, "u", None, 65, 1)
    assert got["count"].max() == 1


@pytest.mark.parametrize("levels", [(1, -1), (0, 1), (1, 1)])
def test_level_ranges_that_leave_holes(ctx, three, levels):
    got, want = scene_sums(ctx, three, "u", "whole", 256, None, *levels)
    assert ref.same_bits(got["covered"], want["covered"])
    start, end = three.rays(256)
    walk = three.wanted("u", 256, None, *levels)
    holes = np.array([(walk["level"][a:b] < 0).any()
                      for a, b in zip(walk["offsets"][:-1], walk["offsets"][1:])])
    d = end - start
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    concerned = holes & (got["status"] == 0)
    if levels[0] == 1:
        assert concerned.sum() > 10
    else:
        assert not holes.any()
    span = ((got["t_leave"] - got["t_enter"]) * length)[concerned]
    assert (got["counted"][concerned] < span).all()


# ---- images --------------------------------------------------------------------------------------------

# the generic direction; the z axis; a direction in the plane z = 2.125, the low z face of the
# level-1 grids (and with an odd height the middle row's rays lie in that plane)
VIEWS = {"generic": ((1.0, 0.7, 0.4), (0.0, 0.0, 1.0), (0.75, -0.25, 2.5)),
         "axis": ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (0.75, -0.25, 2.5)),
         "face": ((1.0, 0.5, 0.0), (0.0, 0.0, 1.0), (0.75, -0.25, 2.125))}
PLANE, DEPTH = (2.0, 1.75), 4.0


@pytest.mark.parametrize("size", [(8, 8), (9, 7), (1, 1), (64, 1)])
@pytest.mark.parametrize("view", ["generic", "axis", "face"])
def test_an_image_is_the_reference_on_the_pixel_rays_in_row_major_order(ctx, three, view, size):
    normal, north, center = VIEWS[view]
    width, height = size
    weight = "whole" if view != "axis" else None
    scene = base.load(ctx, three, "u")
    other = None if weight is None else base.load(ctx, three, weight)
    view = (center, normal, north, PLANE, DEPTH, width, height, three.sizes(), three.lo, three.ratio)
    got = api.project_off_axis_scene(ctx, scene, other, *view)
    tiled = api.project_off_axis_scene(ctx, scene, other, *view, tile_order=True)
    # tile by tile or row by row: the order the rays are walked in does not touch a ray's bits
    assert all((got[key] is None and tiled[key] is None) or
               got[key].tobytes() == tiled[key].tobytes() for key in got)
    start, end = ray_rules.pixel_rays(center, *api.slice_basis(normal, north), PLANE, DEPTH, width,
                                      height)
    want = wanted(three, start, end, "u", weight)
    assert set(got) == {"integral", "weight", "counted", "covered", "status", "count"}
    for key in SUMS + ("status", "count"):
        if want[key] is None:
            assert got[key] is None
            continue
        assert got[key].shape == (height, width) and got[key].dtype == want[key].dtype
        assert got[key].tobytes() == want[key].reshape(height, width).tobytes(), key
    if width * height > 1:
        assert (got["status"] == 0).sum() >= 1
    if view == "face" and height == 7:
        assert (start[3 * width:4 * width, 2] == 2.125).all()       # the middle row, in the face


def defaults(case, min_level=0, max_level=-1):
    """(center, diagonal) of the loaded boxes' bounding box, as project_off_axis works them out."""
    sizes = case.sizes()
    corners = [([case.lo[d] + blo[d] * sizes[l][d] for d in range(3)],
                [case.lo[d] + (bhi[d] + 1) * sizes[l][d] for d in range(3)])
               for l, blo, bhi in case.scene_boxes(min_level, max_level)]
    lo = [min(c[0][d] for c in corners) for d in range(3)]
    hi = [max(c[1][d] for c in corners) for d in range(3)]
    extent = [hi[i] - lo[i] for i in range(3)]
    diagonal = math.sqrt((extent[0] * extent[0] + extent[1] * extent[1]) + extent[2] * extent[2])
    return tuple(0.5 * (lo[i] + hi[i]) for i in range(3)), diagonal


def test_project_off_axis_of_a_plotfile(ctx, three, tmp_path):
    normal = (1.0, 0.7, 0.4)
    picture = str(tmp_path / "offaxis.png")
    api.add_field("uu", "u * u + 1.0")
    got = api.project_off_axis(three.path, normal, variable="u", weight="uu", width=9, height=7,
                               quantity="mean", output=picture)
    assert os.path.getsize(picture) > 0
    # the defaults: the centre of the bounding box, its diagonal as plane_width and depth, north z
    center, diagonal = defaults(three)
    assert center == (0.75, -0.25, 2.5)
    start, end = ray_rules.pixel_rays(center, *api.slice_basis(normal, (0.0, 0.0, 1.0)),
                                      (diagonal, diagonal), diagonal, 9, 7)
    squared = derive_reference.evaluate_levels("u * u + 1.0", three.levels, VARIABLES, three.lo,
                                               three.hi)
    levels = [{"domain": lev["domain"], "boxes": lev["boxes"], "data": [g[None] for g in grids]}
              for lev, grids in zip(three.levels, squared)]
    weight = rr.Hierarchy(levels, three.ratio, 0, three.sizes(), three.lo)
    want = sums_ref.ray_sums(start, end, three.reference("u"), weight)
    with np.errstate(all="ignore"):
        mean = np.where(want["weight"] != 0.0, want["integral"] / want["weight"], math.nan)
    assert got.shape == (7, 9) and ref.same_bits(got, mean.reshape(7, 9))
    assert np.isnan(got).sum() > 0 and np.isfinite(got).sum() > 10
    # a column and an unweighted mean, with a level range
    column = api.project_off_axis(three.path, normal, variable="odd", width=8, height=8, min_level=1)
    mean = api.project_off_axis(three.path, normal, variable="odd", width=8, height=8, min_level=1,
                                quantity="mean")
    center, diagonal = defaults(three, 1, -1)
    assert center == (0.6875, -0.25, 2.375)
    start, end = ray_rules.pixel_rays(center, *api.slice_basis(normal, (0.0, 0.0, 1.0)),
                                      (diagonal, diagonal), diagonal, 8, 8)
    want = wanted(three, start, end, "odd", None, None, 1, -1)
    assert ref.same_bits(column, want["integral"].reshape(8, 8))
    with np.errstate(all="ignore"):
        ratio = np.where(want["counted"] != 0.0, want["integral"] / want["counted"], math.nan)
    assert ref.same_bits(mean, ratio.reshape(8, 8))


# ---- refusals -------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched_and_no_rays_launch_nothing(ctx, three):
    u, whole = base.load(ctx, three, "u"), base.load(ctx, three, "whole")
    cut = base.load(ctx, three, "whole", 1, -1)
    su, sw, sc = (ctx.create_scene(s.local_boxes, s.scalar_transform) for s in (u, whole, cut))
    n = 65
    start_host, end_host = three.rays(n)
    start = torch.from_numpy(start_host).to(ctx.device)
    end = torch.from_numpy(end_host).to(ctx.device)
    out = Buffers(ctx.device, n)
    differ = "the weight scene's boxes differ from the field's"
    shared = "an output array or the rays overlap an input box's cells"
    in_weight = whole.local_boxes[1].values        # an output array that is a weight box's cells
    in_field = u.local_boxes[2].values
    wrong = [
        (dict(weight=sc), differ),                                    # another level range
        (dict(weight=sw, covered=in_weight), shared),
        (dict(weight=sw, weight_out=in_weight), shared),
        (dict(weight=sw, counts=in_weight), shared),
        (dict(weight=sw, end=in_weight), shared),
        (dict(weight=sw, counted=in_field), shared),
        (dict(weight=None, integral=in_field), shared),
        (dict(weight=sw, weight_out=None), "null argument"),          # the null pairs
        (dict(weight=None, weight_out=out.weight), "null argument"),
        (dict(weight=sw, counted=None), "null argument"),
        (dict(weight=None, counts=None), "null argument"),
        (dict(weight=sw, max_trips=0), "max_trips must lie in [1, 2^30]"),
        (dict(weight=sw, n_levels=2), "a box's level is not below n_levels"),
    ]
    for arguments, text in wrong:
        arguments = dict(arguments)
        weight = arguments.pop("weight")
        assert call_sums(ctx, three, su, weight, start, arguments.pop("end", end), out, n_rays=n,
                         **arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert text in _capi.lib().avr_last_error().decode(), (arguments, text)
        ctx.synchronize()
        assert out.untouched(), arguments
    # without the weight scene its cells are no input: the call runs and writes there
    spare = torch.zeros(n, dtype=torch.float64, device=ctx.device)
    assert call_sums(ctx, three, su, None, start, end, out, n_rays=0) == 0
    assert call_sums(ctx, three, su, sw, start, end, out, n_rays=0) == 0
    ctx.synchronize()
    assert out.untouched()                                            # n_rays == 0: no launch
    assert call_sums(ctx, three, su, sw, start, end, out, covered=spare) == 0
    ctx.synchronize()
    got = out.result(True)
    got["covered"] = spare.cpu().numpy()
    same_sums(got, wanted(three, start_host, end_host, "u", "whole"), True)
    assert bool((out.covered == 0.125).all())
    empty = api.ray_sums_scene(ctx, u, np.zeros((0, 3)), np.zeros((0, 3)), three.sizes(), three.lo,
                               three.ratio, whole)
    assert empty["count"].shape == (0,) and empty["weight"].shape == (0,)
    for scene in (su, sw, sc):
        scene.close()
