"""Velocity cubes without a GPU: the numpy reference against a brute-force loop, conservation
against the on-axis projection's reference, closed forms (a linear velocity, one broadened cell
against mpmath), cubes.moments, the FITS writer parsed back by hand, the argument checks of
api.velocity_cube and the new symbol's declaration and binding."""
import math
import os
import struct

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, cubes, runtime

import axis_projection_reference as axis_ref
import velocity_cube_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROB_LO = (0.0, -1.0, 2.0)
PROB_HI = (2.0, 0.5, 3.0)      # 4 x 3 x 2 coarse cells of 0.5: every size is a power of two
EDGES = np.array([-4.0, -1.0, 0.0, 0.75, 3.0, 4.0])


def tiny_levels():
    """4 x 3 x 2 coarse cells, one 4 x 2 x 4 fine grid over two coarse columns.  Components: e
    (small integers with a NaN, a +Inf and a -Inf), g (half-integer lattice in [-5.5, 5.5], one
    NaN), s (0, 0.5, 1 or 3, with a negative and a NaN) and e where g is finite (else NaN)."""
    rng = np.random.default_rng(11)
    boxes = [[((0, 0, 0), (3, 2, 1))], [((2, 2, 0), (5, 3, 3))]]
    domains = [((0, 0, 0), (3, 2, 1)), ((0, 0, 0), (7, 5, 3))]
    levels = []
    for d, bs in zip(domains, boxes):
        data = []
        for lo, hi in bs:
            shape = (hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
            e = rng.integers(-1000, 1001, size=shape).astype(np.float64)
            e.reshape(-1)[rng.choice(e.size, 3, replace=False)] = [np.nan, np.inf, -np.inf]
            g = rng.integers(-6, 6, size=shape).astype(np.float64) + 0.5
            g.reshape(-1)[rng.choice(g.size, 1)] = np.nan
            s = rng.choice([0.0, 0.5, 1.0, 3.0], size=shape)
            s.reshape(-1)[rng.choice(s.size, 2, replace=False)] = [-1.0, np.nan]
            data.append(np.stack([e, g, s, np.where(np.isfinite(g), e, np.nan)]))
        levels.append({"domain": d, "boxes": bs, "data": data})
    return levels


def whole_domain(levels, axis):
    au, av = axis_ref.image_axes(axis)
    center = tuple(0.5 * (PROB_LO[a] + PROB_HI[a]) for a in range(3))
    widths = (PROB_HI[au] - PROB_LO[au], PROB_HI[av] - PROB_LO[av])
    # three pixels per finest cell: no line on a face
    width = 3 * (levels[-1]["domain"][1][au] + 1)
    height = 3 * (levels[-1]["domain"][1][av] + 1)
    assert axis_ref.clearance(levels, PROB_LO, PROB_HI, center, widths, width, height, axis) > 0.1
    return center, widths, width, height


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("s", [None, 2])
def test_reference_equals_the_brute_force_loop(axis, s):
    levels = tiny_levels()
    center, widths, width, height = whole_domain(levels, axis)
    dl = [c[axis] for c in axis_ref.cell_sizes(levels, PROB_LO, PROB_HI)]
    got = ref.reference(levels, PROB_LO, PROB_HI, axis, 0, 1, s, center, widths, width, height, dl,
                        EDGES, with_fsum=True)
    cube, under, over, length = ref.brute_force(levels, PROB_LO, PROB_HI, axis, 0, 1, s, center,
                                                widths, width, height, dl, EDGES)
    assert np.array_equal(got["length"], length) and (got["count"] > 0).any()
    want = np.concatenate([cube, under[None], over[None]])
    have = np.concatenate([got["cube"], got["under"][None], got["over"][None]])
    if s is None:
        # integers and power-of-two sizes: every sum is exact in any order
        assert np.array_equal(have, want) and np.array_equal(got["fsum"], want)
        assert (under != 0).any() and (over != 0).any() and (cube != 0).sum() > 20
    else:
        limit = ref.bound(got["count"], got["abs"]) + 4 * 2.0 ** -53 * got["A"]
        assert (np.abs(have - want) <= limit).all() and (np.abs(got["fsum"] - want) <= limit).all()
        assert (np.abs(have) > 0).sum() > (np.abs(got["fsum"]) > 0).sum() // 2 > 50
    assert (got["abs"] >= np.abs(got["fsum"])).all()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_the_channels_under_and_over_add_up_to_the_projection(axis):
    levels = tiny_levels()
    center, widths, width, height = whole_domain(levels, axis)
    dl = [c[axis] for c in axis_ref.cell_sizes(levels, PROB_LO, PROB_HI)]
    got = ref.reference(levels, PROB_LO, PROB_HI, axis, 0, 1, None, center, widths, width, height,
                        dl, EDGES)
    want = axis_ref.reference(levels, PROB_LO, PROB_HI, axis, 3, None, center, widths, width,
                              height, dl)
    total = got["cube"].sum(axis=0) + got["under"] + got["over"]
    assert np.array_equal(total, want["integral"]) and (total != 0).sum() > 30
    assert np.array_equal(got["length"], want["length"])
    assert np.array_equal(got["count"], want["count"])


def _one_box(n, e, g, s=None):
    """One level, one grid of n cells along z and 1 x 1 across: components e, g, s."""
    data = np.stack([np.broadcast_to(np.asarray(c, np.float64), (n,)).reshape(n, 1, 1)
                     for c in (e, g, 0.0 if s is None else s)])
    return [{"domain": ((0, 0, 0), (0, 0, n - 1)), "boxes": [((0, 0, 0), (0, 0, n - 1))],
             "data": [data]}]


def test_a_uniform_emission_with_a_linear_velocity_fills_channels_by_their_width():
    n = 16
    levels = _one_box(n, 1.0, np.arange(n) + 0.5)
    edges = np.array([0.0, 2.0, 8.0, 13.0])
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 4.0)
    got = ref.reference(levels, lo, hi, 2, 0, 1, None, (0.5, 0.5, 2.0), (1.0, 1.0), 1, 1, [0.25],
                        edges)
    assert np.array_equal(got["cube"][:, 0, 0], 0.25 * np.diff(edges))
    assert got["under"][0, 0] == 0.0 and got["over"][0, 0] == 0.25 * 3 and got["length"][0, 0] == 4.0


def test_one_broadened_cell_matches_erfc_differences_to_forty_digits():
    import mpmath
    mpmath.mp.dps = 40
    edges = np.array([-3.0, -1.25, -0.1, 0.0, 0.3, 0.35, 2.0, 7.5])
    for g, s in ((0.123, 0.75), (-1.3, 0.02), (0.31, 5.0), (6.0, 1.1), (0.3, 1e-3)):
        levels = _one_box(1, 1.0, g, s)
        got = ref.reference(levels, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 2, 0, 1, 2, (0.5, 0.5, 0.5),
                            (1.0, 1.0), 1, 1, [1.0], edges)
        tail = [0.5 * mpmath.erfc((mpmath.mpf(float(x)) - mpmath.mpf(g)) /
                                  (mpmath.mpf(s) * mpmath.sqrt(2))) for x in edges]
        want = [tail[c] - tail[c + 1] for c in range(edges.size - 1)]
        for c, w in enumerate(want):
            assert abs(mpmath.mpf(float(got["cube"][c, 0, 0])) - w) <= 4 * 2.0 ** -53, (g, s, c)
        assert abs(mpmath.mpf(float(got["under"][0, 0])) - (1 - tail[0])) <= 4 * 2.0 ** -53
        assert abs(mpmath.mpf(float(got["over"][0, 0])) - tail[-1]) <= 4 * 2.0 ** -53
        total = got["cube"].sum() + got["under"][0, 0] + got["over"][0, 0]
        assert abs(total - 1.0) <= (edges.size + 3) * 2.0 ** -53


def test_moments_of_a_hand_made_cube():
    edges = np.array([0.0, 2.0, 4.0, 8.0])            # centres 1, 3, 6
    cube = np.zeros((3, 1, 4))
    cube[:, 0, 0] = [2.0, 0.0, 0.0]                   # one channel: centroid 1, dispersion 0
    cube[:, 0, 1] = [1.0, 1.0, 0.0]                   # centroid 2, dispersion 1
    cube[:, 0, 2] = [0.0, 0.0, 0.0]                   # empty: NaN
    cube[:, 0, 3] = [1.0, 0.0, 1.0]                   # centroid 3.5, dispersion 2.5
    m0, m1, m2 = cubes.moments(cube, edges)
    assert np.array_equal(m0, [[2.0, 2.0, 0.0, 2.0]])
    assert np.array_equal(m1[0, [0, 1, 3]], [1.0, 2.0, 3.5]) and np.isnan(m1[0, 2])
    assert np.array_equal(m2[0, [0, 1, 3]], [0.0, 1.0, 2.5]) and np.isnan(m2[0, 2])
    assert np.array_equal(cubes.channel_centers(edges), [1.0, 3.0, 6.0])
    with pytest.raises(ValueError):
        cubes.moments(cube, edges[:3])


def test_combine_velocity_cubes():
    rng = np.random.default_rng(3)
    parts = [(rng.standard_normal((4, 5, 7)),) + tuple(rng.standard_normal((5, 7)) for _ in range(3))
             for _ in range(3)]
    keep = [tuple(a.copy() for a in p) for p in parts]
    for k, got in enumerate(cubes.combine_velocity_cubes(parts)):
        assert np.array_equal(got, (keep[0][k] + keep[1][k]) + keep[2][k])
    assert all(np.array_equal(a, b) for p, q in zip(parts, keep) for a, b in zip(p, q))
    with pytest.raises(ValueError):
        cubes.combine_velocity_cubes([])
    with pytest.raises(ValueError):
        cubes.combine_velocity_cubes([parts[0], tuple(a[..., :4] for a in parts[1])])


def _parse_fits(path):
    raw = open(path, "rb").read()
    assert len(raw) % 2880 == 0
    cards, at = {}, 0
    while True:
        card = raw[at:at + 80].decode("ascii")
        at += 80
        if card.startswith("END"):
            assert card.strip() == "END"
            break
        assert card[8:10] == "= ", card
        value = card[10:].split(" / ")[0].strip()
        cards[card[:8].strip()] = value
    header_bytes = -(-at // 2880) * 2880
    assert set(raw[at:header_bytes]) <= {0x20}
    return cards, raw[header_bytes:]


def test_write_fits_parsed_back_by_hand(tmp_path):
    rng = np.random.default_rng(5)
    cube = rng.standard_normal((4, 3, 5))
    edges = api.bin_edges(-1.5, 2.5, 4)
    path = str(tmp_path / "cube.fits")
    cubes.write_fits(path, cube, edges, (10.0, -2.0), (0.5, 0.25), "y")
    cards, body = _parse_fits(path)
    assert cards["SIMPLE"] == "T" and int(cards["BITPIX"]) == -64 and int(cards["NAXIS"]) == 3
    assert [int(cards[f"NAXIS{i}"]) for i in (1, 2, 3)] == [5, 3, 4]
    assert [cards[f"CTYPE{i}"] for i in (1, 2, 3)] == ["'Z       '", "'X       '", "'VELO    '"]
    assert [float(cards[f"CRPIX{i}"]) for i in (1, 2, 3)] == [1.0, 1.0, 1.0]
    assert [float(cards[f"CRVAL{i}"]) for i in (1, 2, 3)] == [10.25, -1.875, -1.0]
    assert [float(cards[f"CDELT{i}"]) for i in (1, 2, 3)] == [0.5, 0.25, 1.0]
    assert len(body) == 2880 and not any(body[cube.size * 8:])
    back = np.frombuffer(body[:cube.size * 8], dtype=">f8").reshape(cube.shape)
    assert np.array_equal(back, cube)
    assert body[:8] == struct.pack(">d", cube[0, 0, 0])                         # big-endian
    with pytest.raises(ValueError, match="uniformly spaced"):
        cubes.write_fits(path, cube, [0.0, 1.0, 2.0, 3.0, 4.5])
    with pytest.raises(ValueError):
        cubes.write_fits(path, cube[:3], edges)
    # a cube whose data fill whole blocks gets no padding
    cubes.write_fits(path, np.zeros((1, 18, 20)), [0.0, 1.0])
    assert len(_parse_fits(path)[1]) == 2880


def test_write_npz(tmp_path):
    edges = np.array([0.0, 1.0, 3.0])
    cube = np.arange(12.0).reshape(2, 2, 3)
    result = {"cube": cube, "under": cube[0], "over": cube[1], "length": cube[0] + 1, "edges": edges,
              "centers": cubes.channel_centers(edges), "moments": cubes.moments(cube, edges)}
    cubes.write_npz(str(tmp_path / "c.npz"), result)
    back = np.load(tmp_path / "c.npz")
    assert np.array_equal(back["cube"], cube) and np.array_equal(back["edges"], edges)
    assert np.array_equal(back["moment0"], cube.sum(0)) and "moment2" in back


def test_every_argument_check_comes_before_the_plotfile_is_opened():
    missing = "/nonexistent/plotfile"
    good = dict(emission="density", velocity="vz")
    bad = [
        dict(axis="w"), dict(axis=2), dict(emission=None), dict(emission=""), dict(velocity=None),
        dict(velocity=3), dict(width_field=""), dict(width_field=1.0),
        dict(channels=0), dict(channels=1025), dict(channels=2.5), dict(channels=True),
        dict(v_range=(1.0,)), dict(v_range=(2.0, 1.0)), dict(v_range=(1.0, 1.0)),
        dict(v_range=(0.0, float("nan"))), dict(v_range=(0.0, float("inf"))),
        dict(v_range=(1.0, 1.0 + 2.0 ** -50), channels=64),
        dict(edges=[1.0]), dict(edges=[0.0, 0.0]), dict(edges=[0.0, float("nan")]),
        dict(edges=[2.0, 1.0]), dict(edges=list(range(1027))), dict(edges=[[0.0, 1.0]]),
        dict(width=0), dict(height=-3), dict(width=2.5),
        dict(channels=1024, width=2048, height=1024),
        dict(center=(0.0, 1.0)), dict(center=(0.0, float("nan"), 1.0)),
        dict(plane_width=(1.0,)), dict(plane_width=(1.0, 0.0)), dict(plane_width=(-1.0, 1.0)),
        dict(plane_width=(1.0, float("inf"))),
        dict(output="cube.png"), dict(output=3), dict(output="c.fits", edges=[0.0, 1.0, 3.0]),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            api.velocity_cube(missing, **{**good, **kw})
    for kw in (dict(), dict(width_field="sigma", channels=1024, width=16, height=16),
               dict(edges=[0.0, 1.0, 3.0], output="c.npz"), dict(output="C.FITS")):
        with pytest.raises(RuntimeError, match="does not exist"):
            api.velocity_cube(missing, **{**good, **kw})
    center, widths, rng, edges = cubes.validate_cube_arguments(
        "y", "e", "g", "s", 8, (1, 3), None, 8, 4, (1, 2, 3), (4, 5), "out.npz")
    assert center == (1.0, 2.0, 3.0) and widths == (4.0, 5.0) and rng == (1.0, 3.0) and edges is None
    assert np.array_equal(cubes.validate_cube_arguments("z", "e", "g", edges=(0, 1, 4))[3],
                          [0.0, 1.0, 4.0])
    assert np.array_equal(cubes.channel_edges((1.0, 3.0), 4), api.bin_edges(1.0, 3.0, 4))


def test_the_header_declares_the_symbol_and_the_binding_resolves():
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    assert "int avr_scene_velocity_cube(avr_context *ctx, const avr_scene *scene_e" in header
    assert "avr_scene_velocity_cube" in _capi.SIGNATURES
    assert len(_capi.SIGNATURES["avr_scene_velocity_cube"][1]) == 18
    assert getattr(_capi.lib(), "avr_scene_velocity_cube") is not None
    assert getattr(_capi.lib(), "avr_context_set_velocity_cube_scratch_entries") is not None
    assert _capi.lib().avr_abi_version() == 2
    assert hasattr(runtime.Scene, "velocity_cube")
    for name in ("velocity_cube", "velocity_cube_scene"):
        assert callable(getattr(api, name))
    for name in ("validate_cube_arguments", "channel_edges", "combine_velocity_cubes", "moments",
                 "write_npz", "write_fits"):
        assert callable(getattr(cubes, name))
    assert math.erf(6.0) == 1.0                    # the clamp moves q by less than half an ulp
