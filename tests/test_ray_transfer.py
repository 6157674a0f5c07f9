"""Ray transfer without a GPU: ray_transfer_reference held against things that are not itself -- the
closed form for a constant source function at 40 digits, the optically thin limit, the per-ray sums'
integral of the opacity, conservation of the optical depth over the channels, the reversed normal;
transfer.py's functions against literal loops; the api layers with the device work answered by the
reference; and the declared ABI entry."""
import math
import os
import types

import mpmath
import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, runtime, transfer
from amrvolumerenderer_amd import rays as ray_rules

import ray_sums_reference as sums_ref
import ray_transfer_reference as transfer_ref
from test_rays import THREE_BOXES, THREE_DOMAINS, THREE_HI, THREE_LO, Case, generic_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
GENERIC = (1.0, 0.7, 0.4)


@pytest.fixture(scope="module")
def three():
    return Case(THREE_DOMAINS, THREE_BOXES, THREE_LO, THREE_HI, [2, 2], 81)


@pytest.fixture(scope="module")
def walks(three):
    """(start, end, Hierarchy.rays of u and of whole) for 120 generic rays, walked once."""
    start, end = generic_rays(three, 120, 0.0)
    found = [three.hierarchy(c).rays(start, end, three.hierarchy(c).default_max_trips())
             for c in (0, 2)]
    return (start, end, *found)


def with_values(walk, values):
    out = dict(walk)
    out["value"] = np.asarray(values, dtype=np.float64)
    return out


def per_ray(walk):
    return [range(int(a), int(b)) for a, b in zip(walk["offsets"][:-1], walk["offsets"][1:])]


def lengths(start, end, walk):
    """w per segment, as the definition forms it."""
    w = np.zeros(walk["t0"].size)
    for r, cut in enumerate(per_ray(walk)):
        d = [float(end[r, k]) - float(start[r, k]) for k in range(3)]
        length = math.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        for i in cut:
            w[i] = (float(walk["t1"][i]) - float(walk["t0"][i])) * length
    return w


EDGES = np.linspace(-500.0, 500.0, 17)


@pytest.mark.parametrize("scale", [2.0 ** -10, 2.0 ** -3])
@pytest.mark.parametrize("form", ["grey", "sharp", "broadened"])
def test_a_constant_source_has_the_closed_form(walks, form, scale):
    """I[c] = S (1 - exp(-tau[c])) whatever the order and the sizes of the steps."""
    start, end, u, whole = walks
    S = 0.75
    source = with_values(u, np.full(u["value"].size, S))
    opacity = with_values(whole, np.abs(whole["value"]) * scale)
    g = None if form == "grey" else with_values(whole, whole["value"] * 0.5)
    s = with_values(u, 20.0 + 60.0 * np.abs(u["value"])) if form == "broadened" else None
    out = transfer_ref.transfer_of(start, end, source, opacity, g, s,
                                   None if form == "grey" else EDGES)
    mpmath.mp.dps = 40
    worst = 0.0
    for c in range(out["tau"].shape[0]):
        for r in range(start.shape[0]):
            tau = mpmath.mpf(float(out["tau"][c, r]))
            exact = S * (1 - mpmath.exp(-tau))
            # tau itself is a rounded sum of n terms: its error moves the closed form by at most
            # S exp(-tau) n u tau <= S n u / e
            n = int(out["segments"][c, r])
            slack = S * n * U * float(tau * mpmath.exp(-tau))
            error = abs(float(mpmath.mpf(float(out["intensity"][c, r])) - exact))
            bound = float(out["intensity_bound"][c, r]) + slack
            assert error <= bound, (c, r, error, bound)
            if bound > 0.0:
                worst = max(worst, error / bound)
    print("worst error / bound", worst)
    assert out["tau"].max() > (0.5 if form == "grey" else 1e-3)


def test_the_thin_limit_is_the_sum_of_the_emission(walks):
    """a scaled by 2^-40: I[c] = sum S a w rdv to first order, relative to that sum.  A 1 - exp()
    formulation loses every digit here."""
    start, end, u, whole = walks
    opacity = with_values(whole, np.abs(whole["value"]) * 2.0 ** -40)
    g = with_values(whole, whole["value"] * 0.5)
    source = with_values(u, np.abs(u["value"]) + 0.5)        # one sign: the sum does not cancel
    out = transfer_ref.transfer_of(start, end, source, opacity, g, None, EDGES)
    w = lengths(start, end, u)
    rdv = transfer_ref.reciprocal_widths(EDGES)
    checked = 0
    for r, cut in enumerate(per_ray(u)):
        thin = [[] for _ in range(EDGES.size - 1)]
        for i in cut:
            if u["level"][i] < 0:
                continue
            v = float(g["value"][i])
            c = min(int(np.searchsorted(EDGES, v, side="right")) - 1, EDGES.size - 2)
            thin[c].append(float(source["value"][i]) * float(opacity["value"][i]) * w[i] * rdv[c])
        for c, terms in enumerate(thin):
            total = math.fsum(terms)
            if total == 0.0:
                assert out["intensity"][c, r] == 0.0
                continue
            # second order: dtau / 2 and tau in front, both below 1e-8 here; the sum's rounding
            assert abs(out["intensity"][c, r] - total) <= total * (1e-7 + (len(terms) + 8) * U)
            assert abs(out["intensity"][c, r] - total) > 0.0 or len(terms) < 3
            checked += 1
    assert checked > 500
    assert out["tau"].max() < 1e-8


def test_grey_tau_with_a_constant_source_is_the_per_ray_sums_integral_by_bits(walks):
    start, end, u, whole = walks
    opacity = with_values(whole, np.abs(whole["value"]) * 2.0 ** -10)
    out = transfer_ref.transfer_of(start, end, with_values(u, np.ones(u["value"].size)), opacity)
    # (1 a) w and a w have the same bits
    sums = sums_ref.sums_of(start, end, with_values(u, np.ones(u["value"].size)), opacity)
    assert out["tau"][0].tobytes() == sums["integral"].tobytes()
    assert out["tau"][0].tobytes() == sums["weight"].tobytes()
    assert out["counted"].tobytes() == sums["counted"].tobytes()
    assert out["covered"].tobytes() == sums["covered"].tobytes()
    assert out["outside"] is None and out["tau"].max() > 0.5


@pytest.mark.parametrize("form", ["sharp", "broadened"])
def test_the_optical_depth_is_conserved_over_the_channels(walks, form):
    """sum_c tau[c] dv[c] + outside = the integral of a, whatever the channels."""
    start, end, u, whole = walks
    opacity = with_values(whole, np.abs(whole["value"]) * 2.0 ** -10)
    g = with_values(whole, whole["value"] * 0.5)
    s = with_values(u, 1.0 + 90.0 * np.abs(u["value"])) if form == "broadened" else None
    edges = np.linspace(-400.0, 420.0, 34)
    out = transfer_ref.transfer_of(start, end, u, opacity, g, s, edges)
    total = sums_ref.sums_of(start, end, with_values(u, np.ones(u["value"].size)),
                             opacity)["weight"]
    dv = np.diff(edges)
    nc = dv.size
    got = (out["tau"] * dv[:, None]).sum(axis=0) + out["outside"].sum(axis=0)
    n = out["count"].astype(np.float64)
    bound = (2.0 * n + 2.0 + 2.0 * nc) * U * total + 22.0 * U * total
    assert (np.abs(got - total) <= bound).all()
    assert (out["outside"] > 0.0).any(axis=1).all() and total.max() > 0.5


def test_the_reversed_normal_mirrors_tau_and_with_a_constant_source_the_intensity(three):
    center, widths, depth, size = (0.75, -0.25, 2.5), (2.0, 1.75), 4.0, (7, 6)
    north = (0.0, 0.0, 1.0)
    images = []
    for normal in (GENERIC, tuple(-c for c in GENERIC)):
        start, end = ray_rules.pixel_rays(center, *api.slice_basis(normal, north), widths, depth,
                                          *size)
        u, whole = (three.hierarchy(c).rays(start, end, 1000) for c in (0, 2))
        opacity = with_values(whole, np.abs(whole["value"]) * 2.0 ** -10)
        g = with_values(whole, whole["value"] * 0.5)
        images.append(transfer_ref.transfer_of(
            start, end, with_values(u, np.full(u["value"].size, 0.75)), opacity, g, None, EDGES))
    front, back = images
    # seen from behind U flips and V stays: the image is mirrored left to right
    flip = lambda a: a.reshape(a.shape[0], size[1], size[0])[:, :, ::-1].reshape(a.shape[0], -1)
    # the two walks parametrise the same line from either end: every t carries an error of up to
    # 3 u, so a segment's w = (t1 - t0) * length one of up to 7 u * depth, whatever its own size
    n = front["count"].astype(np.float64)
    rdv = max(transfer_ref.reciprocal_widths(EDGES))
    a_max = 1000.0 * 2.0 ** -10
    slack = n * (a_max * 7.0 * U * depth) * rdv + 2.0 * (n + 2.0) * U * front["tau"]
    assert (np.abs(flip(back["tau"]) - front["tau"]) <= slack).all()
    assert (np.abs(flip(back["intensity"]) - front["intensity"]) <=
            0.75 * slack + front["intensity_bound"] + flip(back["intensity_bound"])).all()
    assert flip(back["tau"]).tobytes() != front["tau"].tobytes()     # the order did change
    assert (front["tau"] > 0.0).sum() > 100


# ---- transfer.py ------------------------------------------------------------------------------------

def test_the_background_is_seen_through_the_whole_optical_depth():
    rng = np.random.default_rng(3)
    intensity, tau = rng.random((3, 4, 5)), rng.random((3, 4, 5)) * 5.0
    background = [0.5, 0.0, 2.0]
    got = transfer.apply_background(intensity, tau, background)
    for c in range(3):
        for y in range(4):
            for x in range(5):
                want = intensity[c, y, x] + background[c] * math.exp(-tau[c, y, x])
                assert abs(got[c, y, x] - want) <= 2.0 * U * want
    one = transfer.apply_background(intensity, tau, 1.5)
    assert np.array_equal(one, transfer.apply_background(intensity, tau, [1.5, 1.5, 1.5]))
    assert np.array_equal(transfer.apply_background(intensity, tau, 0.0), intensity)
    for wrong in ([1.0, 2.0], math.nan, [[1.0, 2.0, 3.0]]):
        with pytest.raises(ValueError):
            transfer.apply_background(intensity, tau, wrong)
    with pytest.raises(ValueError):
        transfer.apply_background(intensity, tau[:2], 0.0)


def test_the_line_of_sight_expression_reads_back_as_the_same_floats():
    from amrvolumerenderer_amd import derive
    import derive_reference
    n = api.slice_basis(GENERIC, (0.0, 0.0, 1.0))[0]
    text = transfer.line_of_sight_expression(n, ("vx", "y-velocity", "vz"))
    assert "field('y-velocity')" in text and repr(n[0]) in text
    derive.compile_expression(text, {})
    rng = np.random.default_rng(4)
    v = rng.standard_normal((3, 50))
    got = derive_reference.evaluate(text, {"vx": v[0], "y-velocity": v[1], "vz": v[2]}, {}, (50,))
    want = np.array([-((n[0] * v[0, i] + n[1] * v[1, i]) + n[2] * v[2, i]) for i in range(50)])
    assert got.tobytes() == want.tobytes()
    assert transfer.line_of_sight_values(n, *v).tobytes() == want.tobytes()
    assert (got[v[0] > 5.0 * np.abs(v[1:]).max(axis=0)] < 0.0).all()    # approaching: negative
    assert transfer.velocity_names("vz") == ("vz",)
    assert transfer.velocity_names(["a", "b", "c"]) == ("a", "b", "c")
    for wrong in (("a", "b"), (), 3, ("a", "", "c"), ("a", None, "c")):
        with pytest.raises(ValueError):
            transfer.velocity_names(wrong)
    with pytest.raises(ValueError):
        transfer.line_of_sight_expression((math.nan, 0.0, 1.0), ("a", "b", "c"))


def test_the_arguments_are_checked_before_the_plotfile_is_opened():
    missing = "/nonexistent/plotfile"
    grey = dict(normal=GENERIC, source="S", opacity="a")
    for wrong in (dict(source=""), dict(opacity=None), dict(background=math.inf),
                  dict(background=[1.0, 2.0]), dict(width=0), dict(normal=(0.0, 0.0, 0.0)),
                  dict(depth=-1.0), dict(north=GENERIC), dict(plane_width=(1.0,))):
        with pytest.raises(ValueError):
            api.emission_absorption(missing, **{**grey, **wrong})
    line = dict(normal=GENERIC, source="S", opacity="a", velocity="v")
    for wrong in (dict(velocity=("vx", "vy")), dict(velocity=""), dict(width_field=""),
                  dict(channels=0), dict(channels=1025), dict(v_range=(1.0, 1.0)),
                  dict(edges=[0.0, 0.0, 1.0]), dict(background=[1.0, 2.0]),
                  dict(edges=[0.0, 1.0, 2.0], background=[1.0, math.nan]),
                  dict(output="cube.txt"), dict(edges=[0.0, 1.0, 3.0], output="cube.fits"),
                  dict(channels=1024, width=2048, height=2048), dict(height=-1),
                  dict(normal=(1.0, math.nan, 0.0))):
        with pytest.raises(ValueError):
            api.line_cube(missing, **{**line, **wrong})
    names, rng, edges, background = transfer.validate_line_cube_arguments(
        "S", "a", ("vx", "vy", "vz"), None, 12, (-3.0, 3.0), None, 0.25)
    assert names == ("vx", "vy", "vz") and rng == (-3.0, 3.0) and edges is None
    assert background.tolist() == [0.25] * 12
    _, _, edges, background = transfer.validate_line_cube_arguments(
        "S", "a", "v", "sigma", 64, None, [0.0, 1.0, 4.0], [1.0, 2.0])
    assert edges.tolist() == [0.0, 1.0, 4.0] and background.tolist() == [1.0, 2.0]


def test_several_ranks_are_refused_before_any_device_work(monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(api, "_load_fields", lambda *a, **k: pytest.fail("loaded"))
    with pytest.raises(NotImplementedError):
        api.emission_absorption("/nonexistent", GENERIC, "S", "a")
    with pytest.raises(NotImplementedError):
        api.line_cube("/nonexistent", GENERIC, "S", "a", ("vx", "vy", "vz"))
    assert "_line_of_sight_velocity" not in api.derived_fields()


# ---- the api layers over the reference ---------------------------------------------------------------

def _scene(name):
    return types.SimpleNamespace(name=name, local_boxes=[0], all_boxes=[0], world_scale=1.0)


def _answer_with_the_reference(monkeypatch, case, fields, seen):
    """api.ray_transfer_scene answered by the reference: fields maps a scene's name to values of
    (u's walk, whole's walk)."""
    def fake(ctx, source, opacity, start, end, cell_sizes, prob_lo, ref_ratio, bin_scene=None,
             width_scene=None, edges=None, max_trips=None, rank=0, n_ranks=1):
        u, whole = (case.hierarchy(c).rays(start, end, 1000 if max_trips is None else max_trips)
                    for c in (0, 2))
        walked = [None if s is None else with_values(u, fields[s.name](u["value"], whole["value"]))
                  for s in (source, opacity, bin_scene, width_scene)]
        seen.update(start=start, end=end, edges=edges, max_trips=max_trips)
        out = transfer_ref.transfer_of(start, end, *walked, edges=edges)
        return {key: out[key] for key in ("count", "status", "t_enter", "t_leave", "intensity",
                                          "tau", "outside", "counted", "covered")}
    monkeypatch.setattr(api, "ray_transfer_scene", fake)


FIELDS = {"S": lambda u, whole: u, "a": lambda u, whole: np.abs(whole) * 2.0 ** -10,
          "g": lambda u, whole: whole * 0.5, "s": lambda u, whole: 10.0 + 50.0 * np.abs(u)}


@pytest.mark.parametrize("size", [(9, 7), (1, 1), (64, 1)])
def test_an_image_holds_the_pixel_rays_in_row_major_order(monkeypatch, three, size):
    seen = {}
    _answer_with_the_reference(monkeypatch, three, FIELDS, seen)
    width, height = size
    view = ((0.75, -0.25, 2.5), GENERIC, (0.0, 0.0, 1.0), (2.0, 1.75), 4.0)
    images = api.transfer_off_axis_scene("ctx", _scene("S"), _scene("a"), *view, width, height,
                                         three.sizes, three.lo, three.ratio, _scene("g"),
                                         _scene("s"), EDGES)
    start, end = ray_rules.pixel_rays(view[0], *api.slice_basis(view[1], view[2]), view[3], view[4],
                                      width, height)
    assert seen["start"].tobytes() == start.tobytes() and seen["end"].tobytes() == end.tobytes()
    assert set(images) == {"intensity", "tau", "outside", "counted", "covered", "status", "count"}
    assert images["intensity"].shape == images["tau"].shape == (16, height, width)
    assert images["outside"].shape == (2, height, width)
    assert images["counted"].shape == images["status"].shape == (height, width)
    grey = api.transfer_off_axis_scene("ctx", _scene("S"), _scene("a"), *view, width, height,
                                       three.sizes, three.lo, three.ratio)
    assert grey["outside"] is None and grey["tau"].shape == (1, height, width)
    # the first cell is the nearest: the viewer sits at +n
    assert (((end - start) @ np.array(api.slice_basis(view[1], view[2])[0])) < 0.0).all()
    for wrong in (dict(width=0), dict(depth=0.0), dict(plane_width=(1.0, -1.0))):
        arguments = dict(center=view[0], normal=view[1], north=view[2], plane_width=view[3],
                         depth=view[4], width=width, height=height)
        arguments.update(wrong)
        with pytest.raises(ValueError):
            api.transfer_off_axis_scene("ctx", _scene("S"), _scene("a"), cell_sizes=three.sizes,
                                        prob_lo=three.lo, ref_ratio=three.ratio, **arguments)


def _patched_loader(monkeypatch, three, loaded):
    header = types.SimpleNamespace(cell_size=three.sizes, prob_lo=three.lo, ref_ratio=three.ratio)
    box = types.SimpleNamespace(min_corner=THREE_LO, max_corner=THREE_HI)

    def load(plotfile, variables, min_level, max_level):
        loaded.append((list(variables), dict(api.derived_fields())))
        scenes = [types.SimpleNamespace(name=name, local_boxes=[box], all_boxes=[box],
                                        world_scale=1.0) for name in variables]
        return "ctx", 0, 1, None, scenes, [1.0, 1.0, 1.0]
    monkeypatch.setattr(api, "_load_fields", load)
    from amrvolumerenderer_amd import plotfile as pf
    monkeypatch.setattr(pf, "PlotFileData", lambda path: header)


def test_line_cube_and_emission_absorption_over_the_reference(monkeypatch, three, tmp_path):
    seen, loaded = {}, []
    fields = dict(FIELDS)
    fields["_line_of_sight_velocity"] = FIELDS["g"]
    _answer_with_the_reference(monkeypatch, three, fields, seen)
    _patched_loader(monkeypatch, three, loaded)
    edges = np.linspace(-500.0, 500.0, 9)
    background = np.linspace(0.5, 4.0, 8)
    npz = str(tmp_path / "cube.npz")
    got = api.line_cube("plt", GENERIC, "S", "a", ("vx", "vy", "vz"), width_field="s", edges=edges,
                        background=background, width=6, height=5, output=npz)
    names, registry = loaded[-1]
    assert names == ["S", "a", "_line_of_sight_velocity", "s"]
    unit = api.slice_basis(GENERIC, (0.0, 0.0, 1.0))[0]
    assert registry["_line_of_sight_velocity"] == transfer.line_of_sight_expression(
        unit, ("vx", "vy", "vz"))
    assert "_line_of_sight_velocity" not in api.derived_fields()        # removed again
    assert set(got) == {"cube", "tau", "outside", "counted", "covered", "edges", "centers",
                        "moments"}
    # the defaults: the bounding box's centre, its diagonal as plane_width and as depth
    extent = [h - l for l, h in zip(THREE_LO, THREE_HI)]
    diagonal = math.sqrt((extent[0] * extent[0] + extent[1] * extent[1]) + extent[2] * extent[2])
    center = tuple(0.5 * (l + h) for l, h in zip(THREE_LO, THREE_HI))
    start, end = ray_rules.pixel_rays(center, *api.slice_basis(GENERIC, (0.0, 0.0, 1.0)),
                                      (diagonal, diagonal), diagonal, 6, 5)
    assert seen["start"].tobytes() == start.tobytes() and seen["end"].tobytes() == end.tobytes()
    assert seen["edges"].tobytes() == edges.tobytes() and seen["max_trips"] is None
    # the background rule and the moments, by literal loops
    u, whole = (three.hierarchy(c).rays(start, end, 1000) for c in (0, 2))
    want = transfer_ref.transfer_of(
        start, end, *(with_values(u, FIELDS[k](u["value"], whole["value"])) for k in "Sags"),
        edges=edges)
    assert got["tau"].tobytes() == want["tau"].tobytes()
    assert got["outside"].tobytes() == want["outside"].tobytes()
    for c in range(8):
        for p in range(30):
            value = want["intensity"][c, p] + background[c] * math.exp(-want["tau"][c, p])
            assert abs(got["cube"][c, p // 6, p % 6] - value) <= 2.0 * U * abs(value)
    from amrvolumerenderer_amd import cubes
    moments = cubes.moments(got["cube"] * 125.0, edges)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got["moments"], moments))
    assert got["centers"].tolist() == [0.5 * (edges[c] + edges[c + 1]) for c in range(8)]
    with np.load(npz) as stored:
        assert set(stored.files) == {"cube", "tau", "outside", "counted", "covered", "edges",
                                     "centers", "moment0", "moment1", "moment2"}
        assert stored["tau"].tobytes() == got["tau"].tobytes()
    fits = str(tmp_path / "cube.fits")
    one = api.line_cube("plt", GENERIC, "S", "a", "g", edges=edges, width=6, height=5, output=fits)
    assert loaded[-1][0] == ["S", "a", "g"] and "_line_of_sight_velocity" not in loaded[-1][1]
    raw = open(fits, "rb").read()
    assert len(raw) % 2880 == 0 and b"NAXIS3  =                    8" in raw
    assert np.frombuffer(raw[2880:2880 + 8 * 240], ">f8").tobytes() == \
        one["cube"].astype(">f8").tobytes()
    # a failing load still removes the temporary field
    monkeypatch.setattr(api, "_load_fields", lambda *a, **k: (_ for _ in ()).throw(KeyError("x")))
    with pytest.raises(KeyError):
        api.line_cube("plt", GENERIC, "S", "a", ("vx", "vy", "vz"), edges=edges)
    assert "_line_of_sight_velocity" not in api.derived_fields()


def test_emission_absorption_over_the_reference_and_a_truncated_ray(monkeypatch, three):
    seen, loaded = {}, []
    _answer_with_the_reference(monkeypatch, three, FIELDS, seen)
    _patched_loader(monkeypatch, three, loaded)
    got = api.emission_absorption("plt", GENERIC, "S", "a", background=3.0, width=6, height=5)
    assert loaded[-1][0] == ["S", "a"] and seen["edges"] is None
    assert set(got) == {"intensity", "tau", "counted", "covered"}
    assert all(v.shape == (5, 6) and v.dtype == np.float64 for v in got.values())
    u, whole = (three.hierarchy(c).rays(seen["start"], seen["end"], 1000) for c in (0, 2))
    want = transfer_ref.transfer_of(seen["start"], seen["end"], u,
                                    with_values(u, FIELDS["a"](u["value"], whole["value"])))
    assert got["tau"].tobytes() == want["tau"].tobytes()
    for p in range(30):
        value = want["intensity"][0, p] + 3.0 * math.exp(-want["tau"][0, p])
        assert abs(got["intensity"][p // 6, p % 6] - value) <= 2.0 * U * abs(value)
    assert (got["intensity"][got["counted"] == 0.0] == 3.0).all()
    # a truncated ray names its pixel
    real = api.ray_transfer_scene

    def short(*a, **k):
        out = real(*a, **k)
        out["status"] = out["status"].copy()
        out["status"][2 * 6 + 4] = ray_rules.TRUNCATED
        return out
    monkeypatch.setattr(api, "ray_transfer_scene", short)
    with pytest.raises(RuntimeError, match=r"pixel \(x=4, y=2\)"):
        api.emission_absorption("plt", GENERIC, "S", "a", width=6, height=5)
    with pytest.raises(RuntimeError, match=r"pixel \(x=4, y=2\)"):
        api.line_cube("plt", GENERIC, "S", "a", "g", edges=EDGES, width=6, height=5)


def test_the_entry_is_declared_with_24_arguments_and_the_abi_version_stays(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    declared = header[header.index("int avr_scene_ray_transfer("):]
    declared = declared[:declared.index(";")]
    assert declared.count(",") + 1 == 24
    assert len(_capi.SIGNATURES["avr_scene_ray_transfer"][1]) == 24
    assert len(_capi.SIGNATURES["avr_scene_ray_sums"][1]) == 19
    assert getattr(avr_lib, "avr_scene_ray_transfer") is not None
    assert getattr(avr_lib, "avr_context_set_ray_transfer_chunk") is not None
    assert avr_lib.avr_abi_version() == 2
    assert hasattr(runtime.Scene, "ray_transfer") and hasattr(runtime.Context,
                                                              "set_ray_transfer_chunk")
    for name in ("ray_transfer_scene", "transfer_off_axis_scene", "emission_absorption",
                 "line_cube"):
        assert callable(getattr(api, name))


# ---- an axis view beside the velocity cube ---------------------------------------------------------

@pytest.mark.parametrize("broadened", [False, True])
@pytest.mark.parametrize("ratios", ["2-2"])       # the cube's reference knows ratios of 2 only
def test_an_axis_view_gives_the_velocity_cubes_columns(ratios, broadened):
    """normal z, north y, one pixel per finest-level column: tau[c] dv[c] is the velocity cube of
    e = a along z, whose reference sums the same terms per level and not in walk order.  Extents
    and cell sizes are powers of two: every w is exact."""
    import ray_reference as rr
    import velocity_cube_reference as cube_ref
    from test_rays import AXIS_CASES, AXIS_HI, AXIS_LO
    ratio, domains, boxes, _ = AXIS_CASES[ratios]
    case = Case(domains, boxes, AXIS_LO, AXIS_HI, ratio, 82)
    levels = []
    for lev in case.levels:
        data = [np.stack([np.abs(d[2]) * 2.0 ** -10, d[2] * 0.5, 20.0 + 60.0 * np.abs(d[0])])
                for d in lev["data"]]
        levels.append({"domain": lev["domain"], "boxes": lev["boxes"], "data": data})
    nx, ny, _ = (domains[2][1][d] + 1 for d in range(3))
    center, widths, depth = (1.0, 0.5, 0.5), (2.0, 1.0), 2.0
    start, end = ray_rules.pixel_rays(center, (0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0),
                                      widths, depth, nx, ny)
    a, g, s = (rr.Hierarchy(levels, case.ratio, c, case.sizes, case.lo).rays(start, end, 1000)
               for c in range(3))
    edges = np.linspace(-400.0, 420.0, 34)
    out = transfer_ref.transfer_of(start, end, with_values(a, np.ones(a["value"].size)), a, g,
                                   s if broadened else None, edges)
    dl = [size[2] for size in case.sizes]
    want = cube_ref.reference(levels, AXIS_LO, AXIS_HI, 2, 0, 1, 2 if broadened else None, center,
                              widths, nx, ny, dl, edges, with_fsum=True)
    dv = np.diff(edges)
    n = want["count"].reshape(-1).astype(np.float64)
    total = want["A"].reshape(-1)
    for got, exact, magnitude in (
            (out["tau"] * dv[:, None], want["fsum"][:33].reshape(33, -1),
             want["abs"][:33].reshape(33, -1)),
            (out["outside"], want["fsum"][33:].reshape(2, -1), want["abs"][33:].reshape(2, -1))):
        # the walk's sum, the division by dv and the product with it; broadened: the erf bound
        bound = (2.0 * n + 6.0) * U * magnitude + (22.0 * U * total if broadened else 0.0)
        bad = np.argwhere(~(np.abs(got - exact) <= bound))
        assert bad.size == 0, (bad[:4], [(got[tuple(i)], exact[tuple(i)], bound[tuple(i)], n[i[1]]) for i in bad[:4]])
    assert ref_bits(out["covered"], want["length"].reshape(-1))
    assert (out["tau"] > 0.0).sum() > 1000 and (want["count"] > 4).any()


def ref_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()
