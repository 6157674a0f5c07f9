"""Ray transfer on the GPU: the grey, sharp and broadened modes of avr_rays.hip through
avr_scene_ray_transfer, api.ray_transfer_scene, api.transfer_off_axis_scene, api.emission_absorption
and api.line_cube, against ray_transfer_reference on the segments ray_reference lists.  count,
status, the span, counted and covered are equal by bits; so are tau and outside in the grey and the
sharp form; the intensity -- and, broadened, tau and outside -- are held to the a-priori bounds the
reference computes per ray and channel ("Ray transfer").  The hierarchies and the pool
of 256 rays are test_rays_gpu's and test_off_axis_projection_gpu's; the fields are derived from the
stored u, odd and whole."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, transfer
from amrvolumerenderer_amd import rays as ray_rules
from amrvolumerenderer_amd.renderer import FrameRenderer, RenderParameters

import derive_reference
import gradient_reference as ref
import ray_reference as rr
import ray_transfer_reference as transfer_ref
import test_rays_gpu as base
from test_off_axis_projection_gpu import PLANE, DEPTH, VIEWS

pytestmark = pytest.mark.gpu
VARIABLES = list(ref.VARIABLES)
U = 2.0 ** -53
DV = 31.25                      # the width of a channel where the widths below are given in them

# name -> expression over the stored u, odd (u with NaN and infinities) and whole (integers)
FIELDS = {
    "a_one": "abs(whole) * 0.0009765625",            # 2^-10: optical depths of order 1
    "a_thick": "abs(whole) * 0.125",                 # 2^-3: transmittances underflow
    "a_thin": "abs(whole) * 9.094947017729282e-13",  # 2^-40
    "a_odd": "abs(odd)",
    "one": "whole * 0.0 + 1.0",
    "g": "whole * 0.5",                              # a half-integer lattice in [-500, 500]
    "g_zero": "minimum(whole, -1.0) * 0.0",          # -0.0 everywhere
    "s_zero": "whole * 0.0",                         # +0.0 and -0.0
    # 0.1 to 30 channel widths; one denormal and one of 1e6 widths
    "s_wide": "where(abs(whole) < 20.0, 5e-324, where(abs(whole) > 980.0, 31250000.0, "
              "minimum(0.1 + abs(u) * 10.0, 30.0) * 31.25))",
    "s_odd": "odd * 40.0",                           # negative, NaN and infinite widths
}


@pytest.fixture(autouse=True)
def _registered_fields():
    def clear():
        for name in list(api.derived_fields()):
            api.remove_field(name)
    clear()
    for name, text in FIELDS.items():
        api.add_field(name, text)
    yield
    api._runtime_scope()[0].set_ray_transfer_chunk(0)
    clear()


@pytest.fixture(scope="module")
def three(tmp_path_factory):
    return base._write(tmp_path_factory.mktemp("transfer") / "three", base.THREE_DOMAINS,
                       base.THREE_BOXES, (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 2], 91)


@pytest.fixture(scope="module")
def two_four(tmp_path_factory):
    """The same grids under ratios 2 and 4."""
    domains = [((0, 0, 0), (11, 5, 7)), ((0, 0, 0), (23, 11, 15)), ((0, 0, 0), (95, 47, 63))]
    boxes = [base.THREE_BOXES[0], base.THREE_BOXES[1], [((24, 12, 12), (43, 27, 31))]]
    return base._write(tmp_path_factory.mktemp("transfer") / "two_four", domains, boxes,
                       (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 4], 95)


def hierarchy(case, name, min_level=0, max_level=-1):
    """The reference's hierarchy of a stored or a derived field, made once."""
    if name in VARIABLES:
        return case.reference(name, min_level, max_level)
    key = ("derived", name, min_level, max_level)
    if key not in case.cache:
        grids = derive_reference.evaluate_levels(FIELDS[name], case.levels, VARIABLES, case.lo,
                                                 case.hi)
        levels = [{"domain": lev["domain"], "boxes": lev["boxes"], "data": [g[None] for g in one]}
                  for lev, one in zip(case.levels, grids)]
        case.cache[key] = rr.Hierarchy(levels, case.ratio, 0, case.sizes(), case.lo, min_level,
                                       max_level)
    return case.cache[key]


def walked(case, name, start, end, max_trips=None, min_level=0, max_level=-1):
    """Hierarchy.rays of one field along the rays, computed once per field and set of rays."""
    if name is None:
        return None
    key = ("walk", name, start.tobytes(), end.tobytes(), max_trips, min_level, max_level)
    if key not in case.cache:
        h = hierarchy(case, name, min_level, max_level)
        case.cache[key] = h.rays(start, end, h.default_max_trips() if max_trips is None
                                 else max_trips)
    return case.cache[key]


def wanted(case, start, end, names, edges=None, max_trips=None, min_level=0, max_level=-1):
    """The reference's answer, computed once and left unchanged."""
    key = ("transfer", names, None if edges is None else np.asarray(edges).tobytes(),
           start.tobytes(), end.tobytes(), max_trips, min_level, max_level)
    if key not in case.cache:
        case.cache[key] = transfer_ref.transfer_of(
            start, end, *(walked(case, name, start, end, max_trips, min_level, max_level)
                          for name in names), edges=edges)
    return case.cache[key]


def scenes_of(case, names, min_level=0, max_level=-1):
    """(ctx, the scenes of the names that are not None, in order)."""
    own, rank, world, _, scenes, _ = api._load_fields(case.path, [n for n in names if n], min_level,
                                                      max_level)
    assert (rank, world) == (0, 1)
    found = iter(scenes)
    return own, [None if n is None else next(found) for n in names]


def same_walk(got, want):
    assert got["count"].dtype == np.uint32 and np.array_equal(got["count"], want["count"])
    assert got["status"].dtype == np.uint8 and np.array_equal(got["status"], want["status"])
    for key in ("t_enter", "t_leave", "counted", "covered"):
        assert got[key].dtype == np.float64 and ref.same_bits(got[key], want[key]), key


def within(got, want, bound, what):
    error = np.abs(got - want)
    with np.errstate(all="ignore"):
        ratio = np.where(bound > 0.0, error / bound, np.where(error > 0.0, np.inf, 0.0))
    print(f"{what}: worst error / bound {ratio.max():.3g}, worst error {error.max():.3g}")
    assert np.isfinite(got).all() and (error <= bound).all(), what


def same_transfer(got, want, broadened=False):
    same_walk(got, want)
    assert got["intensity"].shape == want["intensity"].shape
    print("rays:", want["count"].size, "channels:", want["tau"].shape[0], "status:",
          np.bincount(got["status"], minlength=4).tolist())
    if broadened:
        within(got["tau"], want["tau"], want["tau_bound"], "tau")
        n = want["count"].astype(np.float64)
        within(got["outside"], want["outside"],
               U * ((2.0 * n + 4.0) * want["outside"] + 22.0 * want["opacity_sum"]), "outside")
    else:
        assert ref.same_bits(got["tau"], want["tau"])
        assert (got["outside"] is None) == (want["outside"] is None)
        if want["outside"] is not None:
            assert ref.same_bits(got["outside"], want["outside"])
    within(got["intensity"], want["intensity"], want["intensity_bound"], "intensity")


def transfer_rays(case, names, edges=None, n=256, max_trips=None, min_level=0, max_level=-1,
                  chunk=0):
    """api.ray_transfer_scene of the first n rays of the pool beside the reference."""
    own, scenes = scenes_of(case, names, min_level, max_level)
    own.set_ray_transfer_chunk(chunk)
    finest = max(b.level for b in scenes[0].all_boxes)
    start, end = case.rays(n)
    got = api.ray_transfer_scene(own, scenes[0], scenes[1], start, end, case.sizes()[:finest + 1],
                                 case.lo, case.ratio[:finest], scenes[2], scenes[3], edges,
                                 max_trips)
    want = wanted(case, start, end, names, edges, max_trips, min_level, max_level)
    same_transfer(got, want, names[3] is not None)
    return got, want


def edges_of(nc):
    if nc == 1:
        return np.array([-500.0, 500.0])
    if nc == 2:
        return np.array([-500.0, 0.0, 500.0])         # the lattice's first, an inner, its last value
    if nc == 1024:
        return np.linspace(-512.0, 512.0, 1025)       # unit channels: every other g on an edge
    return np.linspace(-400.0, 420.0, nc + 1)         # some of g under, some over


# ---- grey -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["three", "two_four"])
@pytest.mark.parametrize("opacity", ["a_one", "a_thick", "a_thin", "whole"])
def test_grey(request, which, opacity):
    case = request.getfixturevalue(which)
    got, want = transfer_rays(case, ("u", opacity, None, None))
    assert got["status"][:6].tolist() == [0, 1, 1, 3, 3, 3] and (got["status"] == 0).sum() > 150
    walked_rays = got["status"] == 0
    assert (got["tau"][0][walked_rays] > 0.0).sum() > 100
    # rays that miss or are invalid: +0.0
    idle = ~walked_rays
    assert not got["intensity"][0][idle].view(np.uint64).any() and \
        not got["tau"][0][idle].view(np.uint64).any()
    if opacity == "whole":
        assert (got["counted"] < got["covered"]).sum() > 100    # negative cells drop out
    else:
        assert ref.same_bits(got["counted"], got["covered"])
    if opacity == "a_thick":
        assert got["tau"].max() > 30.0


def test_grey_source_and_opacity_with_cells_that_are_not_finite(three):
    got, _ = transfer_rays(three, ("odd", "a_odd", None, None))
    assert (got["counted"] < got["covered"]).sum() > 5


def test_grey_with_a_constant_source_has_the_ray_sums_integral_of_the_opacity(three):
    got, _ = transfer_rays(three, ("one", "a_one", None, None))
    own, scenes = scenes_of(three, ("a_one",))
    start, end = three.rays(256)
    sums = api.ray_sums_scene(own, scenes[0], start, end, three.sizes(), three.lo, three.ratio)
    assert ref.same_bits(got["tau"][0], sums["integral"])
    assert ref.same_bits(got["counted"], sums["counted"])
    # S = 1: I = 1 - exp(-tau) up to the bound, so it never exceeds 1 by more
    assert (got["intensity"] <= 1.0 + 1e-13).all() and got["intensity"].max() > 0.5


# ---- sharp ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nc", [1, 2, 33])
@pytest.mark.parametrize("opacity", ["a_one", "a_thick", "a_thin"])
def test_sharp(three, nc, opacity):
    edges = edges_of(nc)
    names = ("u", opacity, "g", None)
    got, want = transfer_rays(three, names, edges)
    outputs = {key: value.tobytes() for key, value in got.items()}
    # the chunk does not touch a bit
    for chunk in (1, 3):
        other, _ = transfer_rays(three, names, edges, chunk=chunk)
        assert {key: value.tobytes() for key, value in other.items()} == outputs, chunk
    assert (got["tau"] > 0.0).any(axis=1).all()
    if nc == 33:
        assert (got["outside"] > 0.0).any(axis=1).all()
    else:
        assert not got["outside"].any()


def test_sharp_1024_channels(three):
    got, _ = transfer_rays(three, ("u", "a_one", "g", None), edges_of(1024), n=64)
    assert (got["tau"] > 0.0).any(axis=1).sum() > 200
    other, _ = transfer_rays(three, ("u", "a_one", "g", None), edges_of(1024), n=64, chunk=32)
    assert all(got[key].tobytes() == other[key].tobytes() for key in got)


def test_sharp_on_the_ratio_two_four_hierarchy(two_four):
    transfer_rays(two_four, ("odd", "a_odd", "g", None), edges_of(33))


def test_sharp_edges_cases(three):
    # g = -0.0 lies in the channel whose lower edge is 0.0
    got, _ = transfer_rays(three, ("u", "a_one", "g_zero", None), np.array([-1.0, 0.0, 1.0]))
    assert not got["tau"][0].any() and (got["tau"][1] > 0.0).sum() > 150
    # everything under; everything over
    got, want = transfer_rays(three, ("u", "a_one", "g", None), np.array([600.0, 700.0, 800.0]))
    assert not got["tau"].any() and not got["intensity"].any() and not got["outside"][1].any()
    assert ref.same_bits(got["outside"][0], want["opacity_sum"])
    got, want = transfer_rays(three, ("u", "a_one", "g", None), np.array([-800.0, -700.0, -600.0]))
    assert not got["tau"].any() and not got["outside"][0].any()
    assert ref.same_bits(got["outside"][1], want["opacity_sum"])
    # cells on the first, an inner and the last edge: the edges are values the pool meets
    start, end = three.rays(256)
    g = walked(three, "g", start, end)
    values = np.unique(g["value"][g["level"] >= 0])
    edges = np.array([values[0], values[values.size // 2], values[-1]])
    got, _ = transfer_rays(three, ("u", "a_one", "g", None), edges)
    assert not got["outside"].any() and (got["tau"] > 0.0).any(axis=1).all()


# ---- broadened ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("nc", [1, 2, 33])
@pytest.mark.parametrize("opacity", ["a_one", "a_thick", "a_thin"])
def test_broadened(three, nc, opacity):
    edges = np.linspace(-500.0, 500.0, 33)[:nc + 1] if nc < 33 else np.linspace(-500.0, 531.25, 34)
    assert edges[1] - edges[0] == DV
    names = ("u", opacity, "g", "s_wide")
    got, want = transfer_rays(three, names, edges)
    outputs = {key: value.tobytes() for key, value in got.items()}
    for chunk in (1, 3):
        other, _ = transfer_rays(three, names, edges, chunk=chunk)
        assert {key: value.tobytes() for key, value in other.items()} == outputs, chunk
    start, end = three.rays(256)
    s = walked(three, "s_wide", start, end)["value"]
    assert (s == 5e-324).any() and (s == 31250000.0).any()


def test_broadened_with_zero_widths_is_sharp_by_bits(three):
    edges = edges_of(33)
    sharp, _ = transfer_rays(three, ("u", "a_one", "g", None), edges)
    got, _ = transfer_rays(three, ("u", "a_one", "g", "s_zero"), edges)
    assert all(got[key].tobytes() == sharp[key].tobytes() for key in got)


def test_broadened_drops_cells_of_negative_and_nan_width(two_four):
    got, _ = transfer_rays(two_four, ("u", "a_one", "g", "s_odd"), edges_of(33))
    assert (got["counted"] < 0.7 * got["covered"]).sum() > 50


# ---- sizes, truncation, holes, repeats ---------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_the_last_waves_bounds(three, n):
    transfer_rays(three, ("u", "a_one", None, None), n=n)
    transfer_rays(three, ("u", "a_one", "g", "s_wide"), np.linspace(-500.0, 500.0, 33)[:4], n=n,
                  chunk=2)


def test_max_trips_truncates_with_the_partial_sums(three):
    got, _ = transfer_rays(three, ("u", "a_one", "g", None), edges_of(33), max_trips=3)
    assert (got["status"] == 2).sum() > 150 and got["count"].max() <= 3
    assert (got["tau"].sum(axis=0)[got["status"] == 2] > 0.0).any()


@pytest.mark.parametrize("levels", [(1, -1), (0, 1), (1, 1)])
def test_level_ranges_that_leave_holes(three, levels):
    got, _ = transfer_rays(three, ("u", "a_one", "g", None), edges_of(2), min_level=levels[0],
                           max_level=levels[1])
    assert (got["covered"] > 0.0).sum() > 100


def test_a_repeat_gives_equal_bits(three):
    names, edges = ("odd", "a_odd", "g", "s_wide"), np.linspace(-500.0, 500.0, 33)
    first, _ = transfer_rays(three, names, edges)
    again, _ = transfer_rays(three, names, edges)
    assert all(first[key].tobytes() == again[key].tobytes() for key in first)


# ---- the ABI entry -------------------------------------------------------------------------------------

class Buffers:
    """The eight outputs, filled with sentinels."""

    def __init__(self, device, n, nc):
        self.counts = torch.full((n,), -7, dtype=torch.int32, device=device)
        self.status = torch.full((n,), 9, dtype=torch.uint8, device=device)
        self.span = torch.full((n, 2), 0.5, dtype=torch.float64, device=device)
        self.intensity, self.tau = (torch.full((nc, n), 0.125, dtype=torch.float64, device=device)
                                    for _ in range(2))
        self.outside = torch.full((2, n), 0.125, dtype=torch.float64, device=device)
        self.counted, self.covered = (torch.full((n,), 0.125, dtype=torch.float64, device=device)
                                      for _ in range(2))

    def untouched(self):
        return bool((self.counts == -7).all()) and bool((self.status == 9).all()) and \
            bool((self.span == 0.5).all()) and all(
                bool((t == 0.125).all()) for t in (self.intensity, self.tau, self.outside,
                                                   self.counted, self.covered))


def pointer(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def call_transfer(ctx, case, scenes, start, end, out, edges, n_rays=None, max_trips=None,
                  n_levels=None, n_channels=None, **replaced):
    """avr_scene_ray_transfer itself; replaced: arrays by their argument's name."""
    index = np.ascontiguousarray([lo for _, lo, _ in case.scene_boxes()], np.int32)
    ratio = np.ascontiguousarray(case.ratio, np.int32)
    sizes = np.ascontiguousarray(case.sizes(), np.float64)
    prob_lo = np.ascontiguousarray(case.lo, np.float64)
    e = None if edges is None else np.ascontiguousarray(edges, np.float64)
    arrays = dict(counts=out.counts, status=out.status, span=out.span, intensity=out.intensity,
                  tau=out.tau, outside=out.outside if scenes[2] is not None else None,
                  counted=out.counted, covered=out.covered, start=start, end=end)
    arrays.update(replaced)
    torch.cuda.synchronize()      # the fills of torch's stream are done before the context's runs
    return _capi.lib().avr_scene_ray_transfer(
        ctx._handle, *(s._handle if s is not None else None for s in scenes),
        pointer(arrays["start"]), pointer(arrays["end"]),
        int(start.shape[0]) if n_rays is None else n_rays,
        case.reference("u").default_max_trips() if max_trips is None else max_trips,
        index.ctypes.data_as(C.POINTER(C.c_int32)), ratio.ctypes.data_as(C.POINTER(C.c_int32)),
        sizes.ctypes.data_as(C.POINTER(C.c_double)), prob_lo.ctypes.data_as(C.POINTER(C.c_double)),
        len(case.levels) if n_levels is None else n_levels,
        None if e is None else e.ctypes.data_as(C.POINTER(C.c_double)),
        (1 if e is None else e.size - 1) if n_channels is None else n_channels,
        pointer(arrays["counts"]), pointer(arrays["status"]), pointer(arrays["span"]),
        pointer(arrays["intensity"]), pointer(arrays["tau"]), pointer(arrays["outside"]),
        pointer(arrays["counted"]), pointer(arrays["covered"]))


def test_refusals_leave_the_outputs_untouched_and_no_rays_launch_nothing(three):
    ctx, loaded = scenes_of(three, ("u", "a_one", "g", "s_wide"))
    _, (cut,) = scenes_of(three, ("a_one",), 1, -1)
    su, sa, sg, ss, sc = (ctx.create_scene(s.local_boxes, s.scalar_transform)
                          for s in loaded + [cut])
    n, nc = 65, 3
    edges = np.linspace(-500.0, 500.0, 33)[:nc + 1]
    start_host, end_host = three.rays(n)
    start = torch.from_numpy(start_host).to(ctx.device)
    end = torch.from_numpy(end_host).to(ctx.device)
    out = Buffers(ctx.device, n, nc)
    full, sharp, grey = (su, sa, sg, ss), (su, sa, sg, None), (su, sa, None, None)
    shared = "an output array or the rays overlap an input box's cells"
    in_source = loaded[0].local_boxes[2].values
    in_opacity = loaded[1].local_boxes[1].values
    in_bin = loaded[2].local_boxes[0].values
    in_width = loaded[3].local_boxes[1].values
    increasing = edges.copy()
    increasing[2] = increasing[1]
    infinite = edges.copy()
    infinite[3] = math.inf
    wrong = [
        (dict(scenes=(su, sc, sg, ss)), "the opacity scene's boxes differ from the source's"),
        (dict(scenes=(su, sa, sc, ss)), "the bin scene's boxes differ from the source's"),
        (dict(scenes=(su, sa, sg, sc)), "the width scene's boxes differ from the source's"),
        (dict(scenes=full, tau=in_source), shared),
        (dict(scenes=full, intensity=in_opacity), shared),
        (dict(scenes=full, outside=in_bin), shared),
        (dict(scenes=full, covered=in_width), shared),
        (dict(scenes=sharp, end=in_bin), shared),
        (dict(scenes=grey, edges=None, counts=in_opacity), shared),
        (dict(scenes=(su, sa, None, ss)), "null argument"),           # s without g
        (dict(scenes=sharp, edges=None, n_channels=nc), "null argument"),   # g without edges
        (dict(scenes=grey), "null argument"),                         # edges without g
        (dict(scenes=sharp, outside=None), "null argument"),
        (dict(scenes=grey, edges=None, outside=out.outside), "null argument"),
        (dict(scenes=full, tau=None), "null argument"),
        (dict(scenes=full, intensity=None), "null argument"),
        (dict(scenes=grey, edges=None, n_channels=2), "n_channels must be 1 without a bin scene"),
        (dict(scenes=sharp, n_channels=0), "n_channels must lie in [1, 1024]"),
        (dict(scenes=sharp, edges=np.arange(1027.0), n_channels=1025),
         "n_channels must lie in [1, 1024]"),
        (dict(scenes=sharp, edges=increasing), "edges must be strictly increasing"),
        (dict(scenes=sharp, edges=infinite), "edges must be finite"),
        (dict(scenes=full, max_trips=0), "max_trips must lie in [1, 2^30]"),
        (dict(scenes=full, n_levels=2), "a box's level is not below n_levels"),
        (dict(scenes=sharp, n_rays=2 ** 31 // 3 + 1), "2^31 entries or more"),
    ]
    for arguments, text in wrong:
        arguments = dict(arguments)
        scenes = arguments.pop("scenes")
        assert call_transfer(ctx, three, scenes, start, arguments.pop("end", end), out,
                             arguments.pop("edges", edges), **arguments) == \
            _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert text in _capi.lib().avr_last_error().decode(), (arguments, text)
        ctx.synchronize()
        assert out.untouched(), arguments
    assert _capi.lib().avr_context_set_ray_transfer_chunk(ctx._handle, 33) == \
        _capi.AVR_ERR_INVALID_ARGUMENT
    assert call_transfer(ctx, three, full, start, end, out, edges, n_rays=0) == 0
    assert call_transfer(ctx, three, grey, start, end, out, None, n_rays=0) == 0
    ctx.synchronize()
    assert out.untouched()                                            # n_rays == 0: no launch
    # in order: the entry itself beside the reference
    assert call_transfer(ctx, three, full, start, end, out, edges) == 0, \
        _capi.lib().avr_last_error()
    ctx.synchronize()
    host = lambda t: t.cpu().numpy()
    span = host(out.span)
    got = {"count": host(out.counts).view(np.uint32), "status": host(out.status),
           "t_enter": span[:, 0].copy(), "t_leave": span[:, 1].copy(),
           "intensity": host(out.intensity), "tau": host(out.tau), "outside": host(out.outside),
           "counted": host(out.counted), "covered": host(out.covered)}
    same_transfer(got, wanted(three, start_host, end_host, ("u", "a_one", "g", "s_wide"), edges),
                  True)
    empty = api.ray_transfer_scene(ctx, loaded[0], loaded[1], np.zeros((0, 3)), np.zeros((0, 3)),
                                   three.sizes(), three.lo, three.ratio, loaded[2], None, edges)
    assert empty["tau"].shape == (3, 0) and empty["outside"].shape == (2, 0)
    for scene in (su, sa, sg, ss, sc):
        scene.close()


# ---- images and the plotfile layer -------------------------------------------------------------------

def image_reference(case, names, view, width, height, edges=None, min_level=0, max_level=-1):
    center, normal, north, plane, depth = view
    start, end = ray_rules.pixel_rays(center, *api.slice_basis(normal, north), plane, depth, width,
                                      height)
    return wanted(case, start, end, names, edges, None, min_level, max_level)


@pytest.mark.parametrize("size", [(9, 7), (1, 1), (64, 1)])
def test_an_image_is_the_reference_on_the_pixel_rays(three, size):
    normal, north, center = VIEWS["generic"]
    width, height = size
    names, edges = ("u", "a_one", "g", "s_wide"), np.linspace(-500.0, 500.0, 33)[:6]
    own, scenes = scenes_of(three, names)
    got = api.transfer_off_axis_scene(own, scenes[0], scenes[1], center, normal, north, PLANE,
                                      DEPTH, width, height, three.sizes(), three.lo, three.ratio,
                                      scenes[2], scenes[3], edges)
    want = image_reference(three, names, (center, normal, north, PLANE, DEPTH), width, height,
                           edges)
    assert got["intensity"].shape == got["tau"].shape == (5, height, width)
    assert got["outside"].shape == (2, height, width) and got["status"].shape == (height, width)
    flat = {key: value.reshape(value.shape[:-2] + (-1,)) for key, value in got.items()}
    flat["t_enter"], flat["t_leave"] = want["t_enter"], want["t_leave"]     # not part of an image
    same_transfer(flat, want, True)


def defaults(case):
    sizes = case.sizes()
    corners = [([case.lo[d] + blo[d] * sizes[l][d] for d in range(3)],
                [case.lo[d] + (bhi[d] + 1) * sizes[l][d] for d in range(3)])
               for l, blo, bhi in case.scene_boxes()]
    lo = [min(c[0][d] for c in corners) for d in range(3)]
    hi = [max(c[1][d] for c in corners) for d in range(3)]
    extent = [hi[i] - lo[i] for i in range(3)]
    diagonal = math.sqrt((extent[0] * extent[0] + extent[1] * extent[1]) + extent[2] * extent[2])
    return tuple(0.5 * (lo[i] + hi[i]) for i in range(3)), diagonal


def test_emission_absorption_of_a_plotfile(three, tmp_path, monkeypatch):
    normal = (1.0, 0.7, 0.4)
    picture = str(tmp_path / "grey.png")
    got = api.emission_absorption(three.path, normal, "u", "a_one", background=2.5, width=9,
                                  height=7, output=picture)
    assert os.path.getsize(picture) > 0
    assert set(got) == {"intensity", "tau", "counted", "covered"}
    center, diagonal = defaults(three)
    want = image_reference(three, ("u", "a_one", None, None),
                           (center, normal, (0.0, 0.0, 1.0), (diagonal, diagonal), diagonal), 9, 7)
    assert ref.same_bits(got["tau"], want["tau"].reshape(7, 9))
    assert ref.same_bits(got["counted"], want["counted"].reshape(7, 9))
    assert ref.same_bits(got["covered"], want["covered"].reshape(7, 9))
    behind = 2.5 * np.exp(-want["tau"][0])
    error = np.abs(got["intensity"].reshape(-1) - (want["intensity"][0] + behind))
    assert (error <= want["intensity_bound"][0] + 4.0 * U * (np.abs(want["intensity"][0]) + behind)).all()
    assert (got["intensity"][got["counted"] == 0.0] == 2.5).all() and (got["counted"] == 0.0).any()
    monkeypatch.setattr(ray_rules, "default_max_trips", lambda *a: 1)
    with pytest.raises(RuntimeError, match=r"pixel \(x=\d+, y=\d+\)"):
        api.emission_absorption(three.path, normal, "u", "a_one", width=9, height=7)


def test_line_cube_of_a_plotfile(three, tmp_path):
    normal, edges = (1.0, 0.7, 0.4), np.linspace(-300.0, 300.0, 13)
    background = np.linspace(0.0, 1.1, 12)
    unit = api.slice_basis(normal, (0.0, 0.0, 1.0))[0]
    # the three-name velocity against a hand-made derived field
    api.add_field("los", f"-((({unit[0]!r}) * u + ({unit[1]!r}) * u) + ({unit[2]!r}) * whole)")
    FIELDS["los"] = api.derived_fields()["los"]
    try:
        npz, fits = str(tmp_path / "line.npz"), str(tmp_path / "line.fits")
        got = api.line_cube(three.path, normal, "u", "a_one", ("u", "u", "whole"), edges=edges,
                            background=background, width=9, height=7, output=npz)
        by_name = api.line_cube(three.path, normal, "u", "a_one", "los", edges=edges,
                                background=background, width=9, height=7, output=fits)
        assert "_line_of_sight_velocity" not in api.derived_fields()
        assert set(got) == {"cube", "tau", "outside", "counted", "covered", "edges", "centers",
                            "moments"}
        for key in ("cube", "tau", "outside", "counted", "covered", "edges", "centers"):
            assert got[key].tobytes() == by_name[key].tobytes(), key
        center, diagonal = defaults(three)
        want = image_reference(three, ("u", "a_one", "los", None),
                               (center, normal, (0.0, 0.0, 1.0), (diagonal, diagonal), diagonal),
                               9, 7, edges)
        assert ref.same_bits(got["tau"], want["tau"].reshape(12, 7, 9))
        assert ref.same_bits(got["outside"], want["outside"].reshape(2, 7, 9))
        assert (got["tau"] > 0.0).sum() > 100
        behind = background[:, None] * np.exp(-want["tau"])
        error = np.abs(got["cube"].reshape(12, -1) - (want["intensity"] + behind))
        assert (error <= want["intensity_bound"] +
                4.0 * U * (np.abs(want["intensity"]) + behind)).all()
        from amrvolumerenderer_amd import cubes
        moments = cubes.moments(got["cube"] * 50.0, edges)
        assert all(ref.same_bits(a, b) for a, b in zip(got["moments"], moments))
        with np.load(npz) as stored:
            assert stored["cube"].tobytes() == got["cube"].tobytes()
            assert stored["tau"].tobytes() == got["tau"].tobytes()
            assert stored["moment0"].tobytes() == got["moments"][0].tobytes()
        raw = open(fits, "rb").read()
        assert len(raw) % 2880 == 0 and raw.startswith(b"SIMPLE  =")
        # a width field: the broadened form through the same layer
        wide = api.line_cube(three.path, normal, "u", "a_one", "los", width_field="s_wide",
                             edges=edges, width=9, height=7)
        want = image_reference(three, ("u", "a_one", "los", "s_wide"),
                               (center, normal, (0.0, 0.0, 1.0), (diagonal, diagonal), diagonal),
                               9, 7, edges)
        within(wide["tau"].reshape(12, -1), want["tau"], want["tau_bound"], "tau")
        within(wide["cube"].reshape(12, -1), want["intensity"], want["intensity_bound"], "cube")
    finally:
        FIELDS.pop("los", None)


def test_an_off_axis_projection_a_slice_and_a_volume_frame_are_unchanged_around_a_transfer(three):
    ctx = api._runtime_scope()[0]
    scene = base.load(ctx, three, "u")
    camera = api.automatic_camera(scene.bounds)
    params = RenderParameters(120, 72, 0.85, 1, draw_bounds=False)

    def frames():
        column = api.project_off_axis(three.path, (1.0, 0.7, 0.4), variable="u", width=16, height=12)
        cut = api.slice(three.path, 40, 30, "u", axis="y")
        renderer = FrameRenderer(ctx, scene.all_boxes, scene.local_boxes, scene.scalar_transform,
                                 scene.bounds, scene.scalar_range)
        image, rgb8 = renderer.render(params, camera, want_image=True)
        renderer.synchronize()
        out = (column, cut, image.cpu().numpy().copy(), rgb8.cpu().numpy().copy())
        if renderer.native is not None:
            renderer.native.close()
        return out

    before = frames()
    got = api.line_cube(three.path, (1.0, 0.7, 0.4), "u", "a_one", "g", width_field="s_wide",
                        channels=12, v_range=(-500.0, 500.0), width=16, height=12)
    assert (got["tau"] > 0.0).sum() > 500
    after = frames()
    assert ref.same_bits(before[0], after[0]) and ref.same_bits(before[1], after[1])
    assert np.array_equal(before[2].view(np.uint32), after[2].view(np.uint32))
    assert np.array_equal(before[3], after[3]) and before[3].any()
