"""Power spectra without a GPU: the numpy restatement of the transform (fft_reference) against
numpy.fft.fftn within an a-priori bound, exactly on small integers and through Parseval; the bins
against counts from a brute-force loop; the edge rule; spectra's edges, normalisation and .npz
file; the refusals of api.power_spectrum and api.power_spectrum_scene that come before any device
work; the twiddle table of the library and the declarations of the native entries."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, plotfile, spectra
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds

import fft_reference as fr
import gradient_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (1, 1, 2), (2, 1, 4), (8, 4, 2), (4, 8, 16), (1, 2, 1024), (2, 1024, 2),
          (32, 32, 32)]                                   # (nz, ny, nx)
EPS = 2.0 ** -53


def field(shape, seed=5):
    """Random values that span six decades."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 3.0, shape)


# ---- the transform ---------------------------------------------------------------------------------

def test_the_vectorised_reference_is_the_written_out_loops_by_bits():
    rng = np.random.default_rng(1)
    for n in (1, 2, 4, 8, 64):
        re, im = rng.standard_normal(n), rng.standard_normal(n)
        want = fr.fft_line_loops(re, im)
        got = fr.fft_lines(re[None], im[None])
        assert ref.same_bits(got[0][0], want[0]) and ref.same_bits(got[1][0], want[1]), n


@pytest.mark.parametrize("shape", SHAPES)
def test_the_reference_against_fftn_within_the_a_priori_bound(shape):
    """||F - fftn|| <= 32 log2(N) 2^-53 ||fftn||: Higham's bound for Cooley-Tukey with a per-stage
    factor eta = mu + gamma_4 (sqrt 2 + mu), mu <~ 10 * 2^-53 for the twiddles (rounded argument
    plus libm), so eta <~ 16 * 2^-53, doubled for numpy's own error.  Not measured."""
    values = field(shape)
    got = fr.fft3d(values)
    want = np.fft.fftn(values)
    error = np.linalg.norm((got[..., 0] + 1j * got[..., 1] - want).ravel())
    norm = np.linalg.norm(want.ravel())
    bound = 32.0 * math.log2(values.size) * EPS * norm
    print(shape, "error / (2^-53 norm):", error / (EPS * norm), "bound:", bound / (EPS * norm))
    assert got.shape == shape + (2,) and got.dtype == np.float64
    assert error <= bound


def test_small_integers_transform_exactly():
    values = np.arange(8, dtype=np.float64).reshape(2, 2, 2) - 3.0
    got = fr.fft3d(values)
    want = np.zeros((2, 2, 2, 2))
    for kz in range(2):
        for ky in range(2):
            for kx in range(2):
                want[kz, ky, kx, 0] = sum(values[z, y, x] * (-1) ** (kz * z + ky * y + kx * x)
                                          for z in range(2) for y in range(2) for x in range(2))
    assert np.array_equal(got, want) and not np.signbit(got[..., 1]).any()


@pytest.mark.parametrize("shape", [(2, 1, 4), (4, 8, 16)])
def test_parseval(shape):
    values = field(shape, 9)
    spectrum = fr.fft3d(values)
    p = spectrum[..., 0] ** 2 + spectrum[..., 1] ** 2
    mean_square = math.fsum((values ** 2).ravel()) / values.size
    got = math.fsum(p.ravel()) / float(values.size) ** 2
    assert abs(got - mean_square) <= 64.0 * math.log2(values.size) * EPS * mean_square
    # ... and through the bins and the normalisation, with edges that hold every mode
    dims, size = shape[::-1], (0.5, 0.25, 1.0)
    edges = np.array([0.0, 1.0, 5.0, 1e3])
    modes, terms, outside, nonfinite = fr.shell_sums(spectrum, spectra.inverse_length_sq(dims, size),
                                                     spectra.squared_edges(edges))
    power, density, k = spectra.normalise([math.fsum(t) for t in terms], values.size, edges)
    assert outside == 0 and nonfinite == 0 and modes.sum() == values.size
    assert abs(power.sum() - mean_square) <= 64.0 * math.log2(values.size) * EPS * mean_square
    assert np.array_equal(density, power / np.diff(edges)) and np.array_equal(k, [0.5, 3.0, 502.5])


# ---- the bins --------------------------------------------------------------------------------------

def reference_counts(dims, size, edges):
    nx, ny, nz = dims
    spectrum = np.ones((nz, ny, nx, 2))
    modes, _, outside, nonfinite = fr.shell_sums(spectrum, spectra.inverse_length_sq(dims, size),
                                                 spectra.squared_edges(edges))
    assert nonfinite == 0
    return modes.tolist(), outside


@pytest.mark.parametrize("dims, size, modes, outside", [
    ((8, 8, 8), (1.0, 1.0, 1.0), [1, 18, 62, 98, 171], 162),
    ((16, 8, 4), (0.25, 0.5, 1.0), [1, 18, 53], 440),
    ((4, 1, 1), (1.0, 1.0, 1.0), [1, 2, 1], 0),
    ((1, 1, 1), (1.0, 1.0, 1.0), [1], 0)])
def test_default_edges_and_counts_known_from_a_brute_force_loop(dims, size, modes, outside):
    edges = spectra.default_edges(dims, size)
    assert edges.size == len(modes) + 1 and edges[0] == 0.0
    assert fr.brute_force_modes(dims, size, edges) == (modes, outside)
    assert reference_counts(dims, size, edges) == (modes, outside)
    assert sum(modes) + outside == dims[0] * dims[1] * dims[2]


def test_default_edges_are_half_fundamentals_up_to_the_smallest_nyquist():
    edges = spectra.default_edges((16, 8, 4), (0.25, 0.5, 1.0))     # L = 4 everywhere, n = 2
    dk = 2.0 * math.pi / 4.0
    assert edges.tolist() == [0.0, 0.5 * dk, 1.5 * dk, 2.5 * dk]
    edges = spectra.default_edges((8, 1, 2), (1.0, 1.0, 3.0))       # y does not count: L = 8, n = 1
    assert edges.tolist() == [0.0, 0.5 * 2.0 * math.pi / 8.0, 1.5 * 2.0 * math.pi / 8.0]


def test_a_mode_on_an_edge_lands_where_the_rule_says():
    # (nx, ny, nz) = (4, 1, 1) with L = 1: q = m^2 = 0, 1, 4, 1
    spectrum = np.ones((1, 1, 4, 2))
    g = spectra.inverse_length_sq((4, 1, 1), (0.25, 1.0, 1.0))
    assert g[0] == 1.0
    modes, _, outside, _ = fr.shell_sums(spectrum, g, [0.0, 1.0, 4.0])
    assert modes.tolist() == [1, 3] and outside == 0     # E[0] -> bin 0, E[1] -> bin 1, E[n] -> n - 1
    modes, _, outside, _ = fr.shell_sums(spectrum, g, [1.0, 4.0])
    assert modes.tolist() == [3] and outside == 1
    modes, _, outside, _ = fr.shell_sums(spectrum, g, [0.0, 0.5, 1.0])
    assert modes.tolist() == [1, 2] and outside == 1


def test_a_mode_that_is_not_finite_is_counted_before_its_wave_number_is_looked_at():
    spectrum = np.ones((1, 1, 4, 2))
    spectrum[0, 0, 2, 1] = np.inf           # q = 4, outside [0, 1]
    spectrum[0, 0, 1, 0] = np.nan
    modes, terms, outside, nonfinite = fr.shell_sums(spectrum, [1.0, 1.0, 1.0], [0.0, 1.0])
    assert (modes.tolist(), outside, nonfinite) == ([2], 0, 2) and terms == [[2.0, 2.0]]


# ---- spectra.py --------------------------------------------------------------------------------------

def test_squared_edges_and_the_edges_they_refuse():
    e = np.array([0.0, 1.0, 2.5])
    assert np.array_equal(spectra.squared_edges(e), (e / (2.0 * math.pi)) * (e / (2.0 * math.pi)))
    tiny = [0.0, 1e-170, 2e-170]            # in order, but their squares underflow to 0
    assert spectra.check_edges(tiny).tolist() == tiny
    with pytest.raises(ValueError, match="equal once squared"):
        spectra.squared_edges(tiny)
    for wrong in ([1.0], [1.0, 1.0], [2.0, 1.0], [-1.0, 1.0], [0.0, math.inf], [0.0, math.nan],
                  np.arange(2050.0), [[0.0, 1.0]]):
        with pytest.raises(ValueError):
            spectra.squared_edges(wrong)
    assert spectra.squared_edges(np.arange(2049.0)).size == 2049


def test_linear_and_logarithmic_edges_and_the_wave_numbers():
    dims, size = (8, 8, 8), (1.0, 1.0, 1.0)
    default = spectra.default_edges(dims, size)
    assert np.array_equal(spectra.make_edges(dims, size), default)
    linear = spectra.make_edges(dims, size, bins=4, k_range=(0.0, 2.0))
    assert linear.tolist() == [0.0, 0.5, 1.0, 1.5, 2.0]
    log = spectra.make_edges(dims, size, bins=3, k_range=(0.25, 2.0), k_log=True)
    assert np.allclose(log, [0.25, 0.5, 1.0, 2.0], rtol=1e-15, atol=0.0)
    same = spectra.make_edges(dims, size, k_range=(0.5, 1.0))
    assert same.size == default.size and same[0] == 0.5 and same[-1] == 1.0
    for wrong in (dict(k_log=True), dict(bins=0), dict(bins=2049), dict(k_range=(1.0, 1.0)),
                  dict(k_range=(-1.0, 1.0)), dict(k_range=(0.0, 1.0), k_log=True),
                  dict(k_range=(0.0, math.inf))):
        with pytest.raises(ValueError):
            spectra.make_edges(dims, size, **wrong)
    kx, ky, kz = spectra.wave_numbers((4, 1, 2), (0.5, 1.0, 2.0))
    assert np.array_equal(kx, 2.0 * math.pi * np.fft.fftfreq(4, 0.5)) and ky.tolist() == [0.0]
    assert np.array_equal(kz, 2.0 * math.pi * np.fft.fftfreq(2, 2.0))
    for n in (1, 2, 8):
        assert np.array_equal(spectra.signed_modes(n), np.rint(np.fft.fftfreq(n) * n)), n
        assert np.array_equal(fr.signed_modes(n), spectra.signed_modes(n))
    for wrong in ((3, 4, 4), (4, 2048, 4), (4, 4, 0), (4, 4)):
        with pytest.raises(ValueError, match="region|three"):
            spectra.check_dims(wrong)


def test_an_npz_file_gives_back_what_was_saved(tmp_path):
    edges = spectra.default_edges((4, 4, 4), (1.0, 1.0, 1.0))
    power, density, k = spectra.normalise([4.0, 2.0, 1.0], 64, edges)
    one = {"power": power, "spectrum": density, "modes": np.array([1, 18, 26], dtype=np.int64)}
    result = {"level": 1, "lo": (0, -4, 8), "dims": (4, 4, 4), "cell_size": (1.0, 1.0, 1.0),
              "k_edges": edges, "k": k, "fields": {"x velocity": one, "a/b": one},
              "total": power + power, "outside": 19, "nonfinite": 0, "absent": 2}
    path = str(tmp_path / "spectrum.npz")
    spectra.save_npz(result, path)
    assert os.path.exists(path) and not os.path.exists(path + ".npz")
    back = spectra.load_npz(path)
    assert set(back) == set(result) and list(back["fields"]) == ["x velocity", "a/b"]
    for key in ("level", "lo", "dims", "cell_size", "outside", "nonfinite", "absent"):
        assert back[key] == result[key], key
    for key in ("k_edges", "k", "total"):
        assert ref.same_bits(back[key], result[key]), key
    for name in result["fields"]:
        assert ref.same_bits(back["fields"][name]["power"], power)
        assert ref.same_bits(back["fields"][name]["spectrum"], density)
        assert back["fields"][name]["modes"].dtype == np.int64
        assert np.array_equal(back["fields"][name]["modes"], one["modes"])
    assert power.tolist() == [4.0 / 4096.0, 2.0 / 4096.0, 1.0 / 4096.0]


# ---- refusals before any device work -----------------------------------------------------------

DOMAINS = [((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))]
BOXES = [[((0, 0, 0), (15, 7, 7))], [((8, 4, 4), (15, 11, 11))]]
LO, HI, RATIO = (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [2]


def test_api_power_spectrum_refuses_wrong_arguments_before_anything_is_loaded(tmp_path,
                                                                              monkeypatch):
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
    wrong = [dict(region=region, **corners), dict(left_edge=corners["left_edge"]),
             dict(right_edge=corners["right_edge"]), dict(region=((0, 0, 0), (3, -1, 3))),
             dict(region=((0, 0), (3, 3))), dict(level=-1), dict(level=2),
             dict(region=((0, 0, 0), (2, 3, 3))),                     # 3 cells along x
             dict(region=((0, 0, 0), (2047, 3, 3))),                  # 2048 cells along x
             dict(left_edge=(0.0, 0.0, 0.0), right_edge=(0.75, 0.5, 0.5)),   # 6 cells along x
             dict(edges=[0.0, 1.0], bins=3), dict(edges=[0.0, 1.0], k_range=(0.0, 1.0)),
             dict(edges=[0.0, 1.0], k_log=True), dict(edges=[1.0, 0.5]), dict(edges=[-1.0, 0.5]),
             dict(edges=[0.0, math.nan]), dict(edges=[0.0, 1e-170, 2e-170]), dict(edges=[1.0]),
             dict(bins=0), dict(bins=2049), dict(k_log=True), dict(k_range=(2.0, 1.0)),
             dict(k_range=(0.0, 1.0), k_log=True)]
    for arguments in wrong:
        with pytest.raises(ValueError):
            api.power_spectrum(path, **arguments)
    for arguments in (dict(region=((0, 0, 0), (2, 3, 3))), dict(region=((0, 0, 0), (2047, 3, 3)))):
        with pytest.raises(ValueError, match="pass a region"):
            api.power_spectrum(path, **arguments)
    with pytest.raises(RuntimeError):
        api.power_spectrum(str(tmp_path / "none"))
    with pytest.raises(RuntimeError):
        api.power_spectrum(path, fields=["no such field"])
    # ... and what is in order reaches the loader
    for arguments in (dict(), dict(level=0, region=region), dict(level=1, **corners),
                      dict(bins=5, k_range=(0.5, 9.0), k_log=True), dict(edges=[0.0, 1.0, 7.0])):
        with pytest.raises(AssertionError, match="the runtime was touched"):
            api.power_spectrum(path, **arguments)


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
        api.power_spectrum_scene(NoDevice(), full, 0, *arguments, rank=0, n_ranks=2)
    with pytest.raises(NotImplementedError):
        api.power_spectrum_scene(NoDevice(), part, 0, *arguments)
    for level, lo, dims, edges in ((0, (0, 0, 0), (4, 3, 4), None), (0, (0, 0), (4, 4, 4), None),
                                   (0, (0, 0, 0), (4, 2048, 4), None),
                                   (1, (0, 0, 0), (4, 4, 4), None), (-1, (0, 0, 0), (4, 4, 4), None),
                                   (0, (0, 0, 0), (4, 4, 4), [1.0, 0.0]),
                                   (0, (0, 0, 0), (4, 4, 4), [0.0, 1e-170, 2e-170])):
        with pytest.raises(ValueError):
            api.power_spectrum_scene(NoDevice(), full, level, lo, dims, *arguments[2:], edges=edges)


# ---- the library's host side -------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 8, 1024])
def test_the_library_makes_the_twiddle_table_python_makes_by_bits(avr_lib, n):
    table = np.full((n // 2, 2), -7.0)
    assert avr_lib.avr_fft_twiddles(n, table.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert ref.same_bits(table, fr.twiddles(n))
    assert table[0, 0] == 1.0 and table[0, 1] == 0.0 and np.signbit(table[0, 1])   # sin(-0.0)


def test_the_twiddle_entry_refuses_other_lengths(avr_lib):
    table = np.full((1024, 2), -7.0)
    at = table.ctypes.data_as(C.POINTER(C.c_double))
    for n in (1, 0, -2, 3, 12, 2048, 1 << 30):
        assert avr_lib.avr_fft_twiddles(n, at) == _capi.AVR_ERR_INVALID_ARGUMENT, n
        assert avr_lib.avr_last_error().decode() == "n must be a power of two in [2, 1024]"
    assert avr_lib.avr_fft_twiddles(8, None) == _capi.AVR_ERR_INVALID_ARGUMENT
    assert (table == -7.0).all()


def test_the_entries_are_declared_and_exported(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    for name, count in (("avr_fft_twiddles", 2), ("avr_field_fft", 4), ("avr_spectrum_bins", 9)):
        declared = header.split(f"int {name}(")[1].split(");")[0]
        assert len(_capi.SIGNATURES[name][1]) == declared.count(",") + 1 == count, name
        assert getattr(avr_lib, name) is not None
    assert avr_lib.avr_abi_version() == 2
