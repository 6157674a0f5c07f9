"""The inverse transform, the Helmholtz split and the potential without a GPU: the numpy
restatement of the definitions (spectral_reference) through a round trip and against
numpy.fft.ifftn within a-priori bounds; the split on fields whose answer is known without the
reference, and on a random field through the identities S + C = F, kappa . S = 0 and kappa x C = 0;
the potential of a cosine; spectra's .npz files; the refusals of api.helmholtz and api.potential
that come before any device work; the declarations of the native entries."""
import math
import os

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, plotfile, spectra
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds

import fft_reference as fr
import gradient_reference as ref
import spectral_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (nz, ny, nx): the ten shapes of the transform's GPU tests
SHAPES = [(1, 1, 1), (1, 1, 2), (2, 1, 4), (8, 4, 2), (4, 8, 16), (1, 2, 1024), (2, 1024, 2),
          (32, 32, 32), (1024, 1, 2), (1, 1024, 1)]
EPS = 2.0 ** -53


def field(shape):
    """The transform tests' random values, which span six decades."""
    rng = np.random.default_rng(sum(shape))
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 3.0, shape)


def round_trip_bound(n_cells, norm):
    """32 log2(Ntot) 2^-53 ||x||: the per-transform figure 16 log2(Ntot) 2^-53 of DESIGN.md 7,
    "Power spectrum" (Exactness), taken twice.  A-priori, not measured."""
    return 32.0 * math.log2(n_cells) * EPS * norm


# ---- the inverse transform -------------------------------------------------------------------------

def test_the_vectorised_inverse_is_the_written_out_loops_by_bits():
    rng = np.random.default_rng(2)
    for n in (1, 2, 4, 8, 64):
        re, im = rng.standard_normal(n), rng.standard_normal(n)
        table = sr.inverse_twiddles(n)
        want = sr.line_loops(re, im, table)
        got = sr.lines(re[None], im[None], table)
        assert ref.same_bits(got[0][0], want[0]) and ref.same_bits(got[1][0], want[1]), n
        # ... and with the forward table the routine is the forward reference
        forward = sr.lines(re[None], im[None], fr.twiddles(n))
        assert ref.same_bits(forward[0][0], fr.fft_line_loops(re, im)[0]), n
    for n in (2, 8, 1024):
        w, v = fr.twiddles(n), sr.inverse_twiddles(n)
        assert ref.same_bits(v[:, 0], w[:, 0]) and ref.same_bits(v[:, 1], -w[:, 1])
        assert v[0, 1] == 0.0 and not np.signbit(v[0, 1])


@pytest.mark.parametrize("shape", SHAPES)
def test_a_round_trip_gives_the_field_back_within_the_a_priori_bound(shape):
    values = field(shape)
    back, imag = sr.ifft3d(fr.fft3d(values))
    norm = np.linalg.norm(values.ravel())
    error = np.linalg.norm((back - values).ravel())
    left = np.linalg.norm(imag.ravel())
    bound = round_trip_bound(values.size, norm)
    print(shape, "error, imag / (2^-53 norm):", error / (EPS * norm), left / (EPS * norm),
          "bound:", bound / (EPS * norm))
    assert back.shape == shape and imag.shape == shape and back.dtype == np.float64
    assert error <= bound and left <= bound
    if shape == (1, 1, 1):
        assert ref.same_bits(back, values) and imag[0, 0, 0] == 0.0


@pytest.mark.parametrize("shape", SHAPES)
def test_the_inverse_against_ifftn_within_the_a_priori_bound(shape):
    """||x - ifftn|| <= 32 log2(N) 2^-53 ||ifftn||, the forward reference's bound against fftn."""
    spectrum = fr.fft3d(field(shape))
    got, imag = sr.ifft3d(spectrum)
    want = np.fft.ifftn(spectrum[..., 0] + 1j * spectrum[..., 1])
    error = np.linalg.norm((got + 1j * imag - want).ravel())
    norm = np.linalg.norm(want.ravel())
    bound = 32.0 * math.log2(got.size) * EPS * norm
    print(shape, "error / (2^-53 norm):", error / (EPS * norm), "bound:", bound / (EPS * norm))
    assert error <= bound


def test_small_integers_come_back_exactly():
    values = np.arange(8, dtype=np.float64).reshape(2, 2, 2) - 3.0
    back, imag = sr.ifft3d(fr.fft3d(values))
    assert np.array_equal(back, values) and not imag.any()


# ---- the Helmholtz split ---------------------------------------------------------------------------

UNIT = (0.25, 0.25, 0.25)           # h of 4^3 unit cells: every operation below is exact
PROFILE = np.array([1.0, 0.0, -1.0, 0.0])


def exact_cases():
    """{name: ((vx, vy, vz), which part holds everything)} on 4^3."""
    zero = np.zeros((4, 4, 4))
    along_x = zero + 3.0 * PROFILE[None, None, :]
    along_y = zero + 3.0 * PROFILE[None, :, None]
    k, j, i = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
    checker = (-1.0) ** (i + j + k) + 5.0
    return {"a wave along x in vx": ((along_x, zero, zero), "compressive"),
            "a shear along y in vx": ((along_y, zero, zero), "solenoidal"),
            "a checkerboard and a mean": ((checker, checker, checker), "solenoidal")}


def check_exact_split(name, f, solenoidal, compressive):
    """The part that holds everything equals F, the other one is zero everywhere.  A solenoidal
    part equals F by bits.  A compressive part equals F by bits wherever F is not zero, and is a
    zero where F is one -- of either sign: the definition gives C_d = kappa_d * s with s = +0.0
    there, which is -0.0 for a negative kappa_d where F holds +0.0 (the wave along x: the
    imaginary part of the mode kx = 3, m = -1), so equality by bits of the zeros' signs too cannot
    hold together with the definition.  Which zero it is, the comparison with the reference by
    bits on the GPU settles."""
    whole = exact_cases()[name][1]
    for d in range(3):
        if whole == "solenoidal":
            assert solenoidal[d].view(np.uint64).tolist() == f[d].view(np.uint64).tolist(), (name, d)
            assert not compressive[d].any(), (name, d)
        else:
            assert np.array_equal(compressive[d], f[d]), (name, d)
            there = f[d] != 0.0
            assert np.array_equal(compressive[d].view(np.uint64)[there],
                                  f[d].view(np.uint64)[there]), (name, d)
            assert not solenoidal[d].any(), (name, d)


@pytest.mark.parametrize("name", list(exact_cases()))
def test_the_split_of_fields_whose_answer_is_known(name):
    f = [fr.fft3d(v) for v in exact_cases()[name][0]]
    assert any(a.any() for a in f)
    check_exact_split(name, f, *sr.helmholtz(*f, UNIT))


RANDOM_SHAPE, RANDOM_CELLS = (16, 8, 32), (0.5, 0.25, 1.0)


def random_split():
    rng = np.random.default_rng(7)
    velocity = [rng.standard_normal(RANDOM_SHAPE) for _ in range(3)]
    h = spectra.inverse_length(RANDOM_SHAPE[::-1], RANDOM_CELLS)
    f = [fr.fft3d(v) for v in velocity]
    return velocity, f, h, sr.helmholtz(*f, h)


def split_ratios(f, h, solenoidal, compressive):
    """(||S + C - F||, ||kappa . S / |kappa|||, ||kappa x C / |kappa|||) / (2^-53 ||F||)."""
    as_complex = lambda three: np.stack([a[..., 0] + 1j * a[..., 1] for a in three])
    big_f, s, c = as_complex(f), as_complex(solenoidal), as_complex(compressive)
    kappa = np.stack(np.broadcast_arrays(*sr.kappas(f[0].shape[:3], h)))
    length = np.sqrt((kappa * kappa).sum(axis=0))
    unit = np.divide(kappa, length, out=np.zeros_like(kappa), where=length > 0.0)
    scale = EPS * np.linalg.norm(big_f.ravel())
    return (np.linalg.norm((s + c - big_f).ravel()) / scale,
            np.linalg.norm((unit * s).sum(axis=0).ravel()) / scale,
            np.linalg.norm(np.cross(unit, c, axis=0).ravel()) / scale)


def test_the_split_of_a_random_field_keeps_its_identities():
    """Each ratio is at most 8: one unit for each of the at most eight roundings per component
    (three products, two sums, the quotient, the product, the difference)."""
    velocity, f, h, (solenoidal, compressive) = random_split()
    ratios = split_ratios(f, h, solenoidal, compressive)
    print("S + C - F, kappa . S, kappa x C over 2^-53 ||F||:", ratios)
    assert all(r <= 8.0 for r in ratios)
    # real fields come back real: the largest |imag| of the six inverses within the round-trip
    # bound on the field's norm (the projector's norm is 1: neither part is larger than F)
    norm = np.linalg.norm(np.stack(velocity).ravel())
    imag_max = max(np.abs(sr.ifft3d(a)[1]).max() for a in solenoidal + compressive)
    print("imag_max / (2^-53 norm):", imag_max / (EPS * norm))
    assert imag_max <= round_trip_bound(velocity[0].size, norm)
    # ... and the two parts add up to the field
    for d in range(3):
        back = sr.ifft3d(solenoidal[d])[0] + sr.ifft3d(compressive[d])[0]
        assert np.linalg.norm((back - velocity[d]).ravel()) <= \
            round_trip_bound(velocity[0].size, norm) + 8.0 * EPS * norm


def test_the_nyquist_and_mean_modes_count_as_solenoidal():
    assert sr.projector_modes(1).tolist() == [0.0] and sr.projector_modes(2).tolist() == [0.0, 0.0]
    assert sr.projector_modes(4).tolist() == [0.0, 1.0, 0.0, -1.0]
    assert sr.projector_modes(8).tolist() == [0.0, 1.0, 2.0, 3.0, 0.0, -3.0, -2.0, -1.0]
    f = [np.full((2, 2, 2, 2), float(d + 1)) for d in range(3)]       # every q is 0
    f[0][1, 1, 1, 0] = -0.0
    solenoidal, compressive = sr.helmholtz(*f, (1.0, 1.0, 1.0))
    for d in range(3):
        assert solenoidal[d].view(np.uint64).tolist() == f[d].view(np.uint64).tolist()
        assert not compressive[d].any() and not np.signbit(compressive[d]).any()


def test_a_value_that_is_not_finite_propagates_through_its_mode():
    _, f, h, _ = random_split()
    f = [a.copy() for a in f]
    f[1][3, 2, 5, 0] = math.nan
    f[2][0, 0, 0, 1] = math.inf              # the mean mode: kept as it is
    solenoidal, compressive = sr.helmholtz(*f, h)
    for d in range(3):
        assert np.isnan(solenoidal[d][3, 2, 5, 0]) and np.isnan(compressive[d][3, 2, 5, 0])
        assert np.isfinite(solenoidal[d][3, 2, 5, 1]) and np.isfinite(compressive[d][3, 2, 5, 1])
        assert np.isnan(solenoidal[d]).sum() == 1 and np.isnan(compressive[d]).sum() == 1
    assert solenoidal[2][0, 0, 0, 1] == math.inf and not compressive[2][0, 0, 0].any()


# ---- the inverse Laplacian and the potential ---------------------------------------------------

def potential_reference(rho, cells, constant):
    dims = rho.shape[::-1]
    scale = -(constant / (4.0 * math.pi * math.pi))
    spectrum = sr.inverse_laplacian(fr.fft3d(rho), spectra.inverse_length_sq(dims, cells), scale)
    return sr.ifft3d(spectrum)


@pytest.mark.parametrize("shape", [(1, 1, 64), (4, 4, 16)])
def test_the_potential_of_a_cosine(shape):
    cells, constant, amplitude = (0.125, 0.5, 2.0), 3.0, 7.0
    length = shape[2] * cells[0]
    x = (np.arange(shape[2]) + 0.5) * cells[0]
    wave = amplitude * np.cos(2.0 * math.pi * x / length)
    rho = np.zeros(shape) + wave[None, None, :]
    phi, imag = potential_reference(rho, cells, constant)
    want = np.zeros(shape) + (-constant * wave / (2.0 * math.pi / length) ** 2)[None, None, :]
    norm = np.linalg.norm(want.ravel())
    error = np.linalg.norm((phi - want).ravel())
    print(shape, "error / (2^-53 norm):", error / (EPS * norm))
    assert error <= round_trip_bound(rho.size, norm)
    assert np.linalg.norm(imag.ravel()) <= round_trip_bound(rho.size, norm)
    # a mean does not change it, a constant field has none
    shifted, _ = potential_reference(rho + 8.0, cells, constant)
    assert np.linalg.norm((shifted - want).ravel()) <= round_trip_bound(rho.size, norm)
    flat, flat_imag = potential_reference(np.full(shape, 2.5), cells, constant)
    assert not flat.any() and not flat_imag.any()


def test_the_inverse_laplacian_divides_by_the_shell_sums_q():
    spectrum = np.ones((1, 2, 4, 2))
    spectrum[0, 0, 0] = (5.0, math.nan)                  # the mean mode: (+0, +0) whatever it held
    g = spectra.inverse_length_sq((4, 2, 1), (0.25, 0.25, 1.0))      # L = (1, 0.5, 1): g = (1, 4, 1)
    got = sr.inverse_laplacian(spectrum, g, -2.0)
    q = np.array([[0.0, 1.0, 4.0, 1.0], [4.0, 5.0, 8.0, 5.0]])
    want = np.zeros((1, 2, 4, 2))
    want[0][q > 0.0] = (-2.0 / q[q > 0.0])[:, None]
    assert got.view(np.uint64).tolist() == want.view(np.uint64).tolist()


# ---- spectra.py --------------------------------------------------------------------------------------

def test_the_inverse_lengths_and_the_compressive_fraction():
    assert spectra.inverse_length((4, 4, 4), (1.0, 1.0, 1.0)).tolist() == [0.25, 0.25, 0.25]
    assert spectra.inverse_length((16, 8, 2), (0.5, 0.25, 1.0)).tolist() == [0.125, 0.5, 0.5]
    edges = [0.0, 1.0, 2.0, 3.0]
    assert spectra.compressive_fraction([100.0, 3.0, 1.0], [50.0, 1.0, 3.0], edges) == 0.5
    assert spectra.compressive_fraction([100.0, 3.0, 1.0], [50.0, 1.0, 3.0], [0.5, 1.0, 2.0, 3.0]) \
        == 54.0 / 158.0
    assert math.isnan(spectra.compressive_fraction([1.0], [1.0], [0.0, 1.0]))


def test_the_npz_files_give_back_what_was_saved(tmp_path):
    edges = spectra.default_edges((4, 4, 4), (1.0, 1.0, 1.0))
    power, density, k = spectra.normalise([4.0, 2.0, 1.0], 64, edges)
    modes = np.array([3, 54, 78], dtype=np.int64)
    grid = np.arange(64.0).reshape(4, 4, 4)
    result = {"level": 1, "lo": (0, -4, 8), "dims": (4, 4, 4), "cell_size": (1.0, 1.0, 1.0),
              "k_edges": edges, "k": k,
              "power": {"solenoidal": power, "compressive": 2.0 * power, "total": 3.0 * power},
              "spectrum": {"solenoidal": density, "compressive": 2.0 * density,
                           "total": 3.0 * density},
              "modes": {"solenoidal": modes, "compressive": modes},
              "compressive_fraction": 2.0 / 3.0, "imag_max": 1e-17,
              "solenoidal": {"x velocity": grid, "a/b": -grid, "w": grid + 0.5},
              "compressive": {"x velocity": 2.0 * grid, "a/b": grid, "w": grid - 0.5},
              "outside": 19, "nonfinite": 0, "absent": 2}
    path = str(tmp_path / "split.npz")
    spectra.save_helmholtz_npz(result, path)
    assert os.path.exists(path) and not os.path.exists(path + ".npz")
    back = spectra.load_helmholtz_npz(path)
    assert set(back) == set(result)
    for key in ("level", "lo", "dims", "cell_size", "outside", "nonfinite", "absent",
                "compressive_fraction", "imag_max"):
        assert back[key] == result[key] and type(back[key]) is type(result[key]), key
    assert ref.same_bits(back["k_edges"], edges) and ref.same_bits(back["k"], k)
    for key in ("power", "spectrum", "modes", "solenoidal", "compressive"):
        assert list(back[key]) == list(result[key]), key
        for name in result[key]:
            assert back[key][name].dtype == result[key][name].dtype
            assert np.array_equal(back[key][name], result[key][name]), (key, name)
    # without the grids
    less = {key: value for key, value in result.items()
            if key not in ("solenoidal", "compressive", "imag_max")}
    spectra.save_helmholtz_npz(less, path)
    assert set(spectra.load_helmholtz_npz(path)) == set(less)

    phi = {"level": 0, "lo": (0, 0, 0), "dims": (4, 4, 4), "cell_size": (0.5, 0.25, 1.0),
           "constant": -2.5, "potential": grid, "imag_max": 0.0, "absent": 0}
    path = str(tmp_path / "potential.npz")
    spectra.save_potential_npz(phi, path)
    back = spectra.load_potential_npz(path)
    assert set(back) == set(phi) and ref.same_bits(back["potential"], grid)
    for key in ("level", "lo", "dims", "cell_size", "constant", "imag_max", "absent"):
        assert back[key] == phi[key] and type(back[key]) is type(phi[key]), key


# ---- refusals before any device work -----------------------------------------------------------

DOMAINS = [((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))]
BOXES = [[((0, 0, 0), (15, 7, 7))], [((8, 4, 4), (15, 11, 11))]]
LO, HI, RATIO = (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [2]
VELOCITY = ["u", "whole", "u"]


def test_the_api_refuses_wrong_arguments_before_anything_is_loaded(tmp_path, monkeypatch):
    path = str(tmp_path / "plt")
    plotfile.write_plotfile(path, list(ref.VARIABLES), ref.make_levels(DOMAINS, BOXES, RATIO, 3),
                            LO, HI, RATIO)

    def untouched(*args, **kwargs):
        raise AssertionError("the runtime was touched")

    monkeypatch.setattr(api, "_runtime_scope", untouched)
    monkeypatch.setattr(api, "_ensure_runtime", untouched)
    monkeypatch.setattr(api, "_load_variable_scenes", untouched)
    region = ((0, 0, 0), (3, 3, 3))
    corners = dict(left_edge=(0.0, 0.0, 0.0), right_edge=(0.5, 0.5, 0.5))
    grid_wrong = [dict(region=region, **corners), dict(left_edge=corners["left_edge"]),
                  dict(right_edge=corners["right_edge"]), dict(region=((0, 0, 0), (3, -1, 3))),
                  dict(region=((0, 0), (3, 3))), dict(level=-1), dict(level=2),
                  dict(region=((0, 0, 0), (2, 3, 3))),                     # 3 cells along x
                  dict(region=((0, 0, 0), (2047, 3, 3))),                  # 2048 cells along x
                  dict(left_edge=(0.0, 0.0, 0.0), right_edge=(0.75, 0.5, 0.5))]   # 6 along x
    bins_wrong = [dict(edges=[0.0, 1.0], bins=3), dict(edges=[0.0, 1.0], k_range=(0.0, 1.0)),
                  dict(edges=[0.0, 1.0], k_log=True), dict(edges=[1.0, 0.5]),
                  dict(edges=[-1.0, 0.5]), dict(edges=[0.0, math.nan]),
                  dict(edges=[0.0, 1e-170, 2e-170]), dict(edges=[1.0]), dict(bins=0),
                  dict(bins=2049), dict(k_log=True), dict(k_range=(2.0, 1.0)),
                  dict(k_range=(0.0, 1.0), k_log=True)]
    for arguments in grid_wrong + bins_wrong:
        with pytest.raises(ValueError):
            api.helmholtz(path, VELOCITY, **arguments)
    for arguments in grid_wrong + [dict(constant=math.inf), dict(constant=math.nan)]:
        with pytest.raises(ValueError):
            api.potential(path, "u", **arguments)
    for velocity in (["u"], ["u", "whole"], ["u"] * 4, "u", []):
        with pytest.raises(ValueError, match="three components"):
            api.helmholtz(path, velocity)
    for arguments in (dict(region=((0, 0, 0), (2, 3, 3))), dict(region=((0, 0, 0), (2047, 3, 3)))):
        with pytest.raises(ValueError, match="pass a region"):
            api.helmholtz(path, VELOCITY, **arguments)
        with pytest.raises(ValueError, match="pass a region"):
            api.potential(path, "u", **arguments)
    with pytest.raises(RuntimeError):
        api.helmholtz(str(tmp_path / "none"), VELOCITY)
    with pytest.raises(RuntimeError):
        api.potential(str(tmp_path / "none"), "u")
    with pytest.raises(RuntimeError):
        api.helmholtz(path, ["u", "no such field", "whole"])
    with pytest.raises(RuntimeError):
        api.potential(path, "no such field")
    # ... and what is in order reaches the loader
    for arguments in (dict(), dict(level=0, region=region), dict(level=1, **corners),
                      dict(bins=5, k_range=(0.5, 9.0), k_log=True), dict(edges=[0.0, 1.0, 7.0]),
                      dict(grids=False)):
        with pytest.raises(AssertionError, match="the runtime was touched"):
            api.helmholtz(path, VELOCITY, **arguments)
    for arguments in (dict(), dict(level=0, region=region), dict(level=1, **corners),
                      dict(constant=-4.0)):
        with pytest.raises(AssertionError, match="the runtime was touched"):
            api.potential(path, "u", **arguments)


def test_boxes_on_other_ranks_and_wrong_arguments_are_refused_before_device_work():
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"the context was used ({name})")

    box = AmrBox((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), level=0, dims=(4, 4, 4))
    bounds = VolumeBounds((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    full = api.SceneGeometry([box, box], [box, box], ScalarTransform(), bounds)
    part = api.SceneGeometry([box, box], [box], ScalarTransform(), bounds)
    arguments = ((0, 0, 0), (4, 4, 4), [(0.25, 0.25, 0.25)], (0.0, 0.0, 0.0), [])
    with pytest.raises(NotImplementedError):
        api.helmholtz_scene(NoDevice(), full, full, full, 0, *arguments, rank=0, n_ranks=2)
    with pytest.raises(NotImplementedError):
        api.potential_scene(NoDevice(), full, 0, *arguments, rank=0, n_ranks=2)
    for three in ((part, full, full), (full, part, full), (full, full, part)):
        with pytest.raises(NotImplementedError):
            api.helmholtz_scene(NoDevice(), *three, 0, *arguments)
    with pytest.raises(NotImplementedError):
        api.potential_scene(NoDevice(), part, 0, *arguments)
    for level, lo, dims, edges in ((0, (0, 0, 0), (4, 3, 4), None), (0, (0, 0), (4, 4, 4), None),
                                   (0, (0, 0, 0), (4, 2048, 4), None),
                                   (1, (0, 0, 0), (4, 4, 4), None), (-1, (0, 0, 0), (4, 4, 4), None),
                                   (0, (0, 0, 0), (4, 4, 4), [1.0, 0.0]),
                                   (0, (0, 0, 0), (4, 4, 4), [0.0, 1e-170, 2e-170])):
        with pytest.raises(ValueError):
            api.helmholtz_scene(NoDevice(), full, full, full, level, lo, dims, *arguments[2:],
                                edges=edges)
        if edges is None:
            with pytest.raises(ValueError):
                api.potential_scene(NoDevice(), full, level, lo, dims, *arguments[2:])
    with pytest.raises(ValueError, match="constant"):
        api.potential_scene(NoDevice(), full, 0, *arguments, constant=math.inf)


# ---- the library's host side -------------------------------------------------------------------------

def test_the_entries_are_declared_and_exported(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    for name, count in (("avr_field_ifft", 5), ("avr_spectrum_helmholtz", 5),
                        ("avr_spectrum_inverse_laplacian", 5)):
        declared = header.split(f"int {name}(")[1].split(");")[0]
        assert len(_capi.SIGNATURES[name][1]) == declared.count(",") + 1 == count, name
        assert getattr(avr_lib, name) is not None
    assert avr_lib.avr_abi_version() == 2
