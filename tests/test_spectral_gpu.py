"""The inverse transform, the Helmholtz split and the potential on the GPU: ifft_x_kernel and the
kernels of avr_spectral.hip through avr_field_ifft, avr_spectrum_helmholtz and
avr_spectrum_inverse_laplacian, Context.ifft3d, Context.helmholtz_split and
Context.inverse_laplacian, api.helmholtz and api.potential, against the numpy restatement of the
definitions (spectral_reference).  Everything but the bins is equal by bits; the bins' counts are
equal and their sums lie within the a-priori bound of adding non-negative terms in any order around
a math.fsum reference."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, plotfile, spectra

import covering_grid_reference as cg
import fft_reference as fr
import gradient_reference as ref
import spectral_reference as sr
from test_spectral import UNIT, check_exact_split, exact_cases

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
# (nz, ny, nx): a length-1 axis, a line shorter than a wave, the longest contiguous line, both
# strided passes, odd and even log2, nx below the column group; the last two are the longest
# strided lines with a partial column group
SHAPES = [(1, 1, 1), (1, 1, 2), (2, 1, 4), (8, 4, 2), (4, 8, 16), (1, 2, 1024), (2, 1024, 2),
          (32, 32, 32), (1024, 1, 2), (1, 1024, 1)]
# of the per-mode kernels: one mode, a partial trip, several trips, a second workgroup (16384
# modes each) with a partial last one, every axis with a Nyquist mode and without
MODE_SHAPES = [(1, 1, 1), (2, 1, 4), (8, 4, 2), (4, 8, 16), (32, 32, 32), (2, 1024, 2)]
SIZE = (0.5, 0.25, 1.0)          # (dx, dy, dz)


def random_field(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 3.0, shape)


@functools.lru_cache(maxsize=None)
def spectra_of(shape):
    """Three spectra of a shape, the transforms of six-decade random fields, made once; treat
    them as read-only."""
    return tuple(fr.fft3d(random_field(shape, sum(shape) + d)) for d in range(3))


@functools.lru_cache(maxsize=None)
def inverse_of(shape):
    return sr.ifft3d(spectra_of(shape)[0])


def on_device(ctx, array):
    return torch.from_numpy(np.ascontiguousarray(array)).to(ctx.device)


def differing(got, want):
    return np.argwhere(np.ascontiguousarray(got).view(np.uint64) !=
                       np.ascontiguousarray(want).view(np.uint64))


# ---- 1. the inverse transform ----------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_ifft3d_equals_the_reference_by_bits(ctx, shape):
    spectrum = spectra_of(shape)[0]
    want_real, want_imag = inverse_of(shape)
    real, imag = ctx.ifft3d(on_device(ctx, spectrum), with_imag=True)
    alone = ctx.ifft3d(on_device(ctx, spectrum))
    ctx.synchronize()
    assert isinstance(alone, torch.Tensor) and alone.shape == shape and alone.dtype == torch.float64
    for got, want in ((real, want_real), (imag, want_imag), (alone, want_real)):
        different = differing(got.cpu().numpy(), want)
        print(shape, "differing cells:", len(different), different[:4].tolist())
        assert got.shape == shape and len(different) == 0


def test_a_round_trip_of_small_integers_is_exact(ctx):
    values = np.arange(8, dtype=np.float64).reshape(2, 2, 2) - 3.0
    real, imag = ctx.ifft3d(ctx.fft3d(on_device(ctx, values)), with_imag=True)
    ctx.synchronize()
    assert np.array_equal(real.cpu().numpy(), values) and not imag.cpu().numpy().any()


def test_ifft3d_takes_contiguous_float64_spectra_only(ctx):
    spectrum = on_device(ctx, spectra_of((4, 8, 16))[0])
    for wrong in (spectrum.float(), spectrum[:, :, ::2], spectrum[..., 0], spectrum[0],
                  spectrum.cpu()):
        with pytest.raises(ValueError):
            ctx.ifft3d(wrong)
    for shape in ((4, 8, 12, 2), (4, 8, 2048, 2)):
        with pytest.raises(ValueError, match="dims must be powers of two"):
            ctx.ifft3d(torch.zeros(shape, dtype=torch.float64, device=ctx.device))


# ---- 2. the Helmholtz split ------------------------------------------------------------------------

def split_on_device(ctx, f, h):
    inputs = [on_device(ctx, a) for a in f]
    solenoidal, compressive = ctx.helmholtz_split(*inputs, h)
    ctx.synchronize()
    assert all(s.data_ptr() == a.data_ptr() for s, a in zip(solenoidal, inputs))   # overwritten
    return [t.cpu().numpy() for t in solenoidal], [t.cpu().numpy() for t in compressive]


def check_split(got, want, what):
    for part, got_part, want_part in zip(("solenoidal", "compressive"), got, want):
        for d in range(3):
            different = differing(got_part[d], want_part[d])
            print(what, part, d, "differing components:", len(different), different[:4].tolist())
            assert got_part[d].shape == want_part[d].shape and len(different) == 0


@pytest.mark.parametrize("shape", MODE_SHAPES)
def test_helmholtz_split_equals_the_reference_by_bits(ctx, shape):
    h = spectra.inverse_length(shape[::-1], SIZE)
    f = spectra_of(shape)
    check_split(split_on_device(ctx, f, h), sr.helmholtz(*f, h), shape)


@pytest.mark.parametrize("name", list(exact_cases()))
def test_the_split_of_fields_whose_answer_is_known(ctx, name):
    f = [fr.fft3d(v) for v in exact_cases()[name][0]]
    got = split_on_device(ctx, f, np.array(UNIT))
    check_split(got, sr.helmholtz(*f, UNIT), name)
    check_exact_split(name, f, *got)


def test_one_nan_cell_propagates_as_the_reference_says(ctx):
    shape = (4, 8, 16)
    h = spectra.inverse_length(shape[::-1], SIZE)
    fields = [random_field(shape, 40 + d) for d in range(3)]
    fields[1][1, 2, 3] = math.nan
    f = [fr.fft3d(v) for v in fields]
    got = [ctx.fft3d(on_device(ctx, v)) for v in fields]
    solenoidal, compressive = ctx.helmholtz_split(*got, h)
    ctx.synchronize()
    want = sr.helmholtz(*f, h)
    for got_part, want_part in zip((solenoidal, compressive), want):
        for d in range(3):
            assert ref.same_bits(got_part[d].cpu().numpy(), want_part[d])
    # vy is NaN in every mode, and so is every part of every mode but the mean and Nyquist ones,
    # where the other two components pass through
    assert np.isnan(want[0][1]).all() and np.isnan(want[1][0]).sum() == 2 * (4 * 8 * 16 - 8)
    assert np.isfinite(want[0][0][0, 0, 0]).all() and not want[1][0][2, 4, 8].any()


def test_helmholtz_split_takes_three_spectra_of_one_shape(ctx):
    f = [on_device(ctx, a) for a in spectra_of((4, 8, 16))]
    with pytest.raises(ValueError, match="one shape"):
        ctx.helmholtz_split(f[0], f[1], on_device(ctx, spectra_of((8, 4, 2))[0]), (1.0, 1.0, 1.0))
    with pytest.raises(ValueError, match="three values"):
        ctx.helmholtz_split(*f, (1.0, 1.0))
    with pytest.raises(ValueError):
        ctx.helmholtz_split(f[0], f[1], f[2].float(), (1.0, 1.0, 1.0))


# ---- 3. the inverse Laplacian ----------------------------------------------------------------------

@pytest.mark.parametrize("shape", MODE_SHAPES)
def test_inverse_laplacian_equals_the_reference_by_bits(ctx, shape):
    g = spectra.inverse_length_sq(shape[::-1], SIZE)
    spectrum = spectra_of(shape)[0]
    for scale in (0.7, -3.0 / (4.0 * math.pi * math.pi)):
        on = on_device(ctx, spectrum)
        got = ctx.inverse_laplacian(on, g, scale)
        ctx.synchronize()
        assert got.data_ptr() == on.data_ptr()                         # in place
        different = differing(got.cpu().numpy(), sr.inverse_laplacian(spectrum, g, scale))
        print(shape, scale, "differing components:", len(different), different[:4].tolist())
        assert len(different) == 0
        assert not got[0, 0, 0].any() and not torch.signbit(got[0, 0, 0]).any()


# ---- 4. the API ------------------------------------------------------------------------------------

DOMAINS = [((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))]
BOXES = [[((0, 0, 0), (15, 7, 7))], [((8, 4, 4), (15, 11, 11))]]
LO, HI, RATIO = (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [2]
NAMES = ["vx", "vy", "vz", "rho"]
VELOCITY = NAMES[:3]


class Plot:
    """A 16 x 8 x 8 plotfile with one finer patch and four finite fields: gradient_reference's
    levels made twice, of each its normal and its integer field (the cells under the patch hold
    1e30 in all of them)."""

    def __init__(self, path):
        self.path = str(path)
        first, second = (ref.make_levels(DOMAINS, BOXES, RATIO, seed) for seed in (83, 84))
        self.levels = [{"domain": a["domain"], "boxes": a["boxes"],
                        "data": [np.stack([x[0], y[0], x[2], y[2]])
                                 for x, y in zip(a["data"], b["data"])]}
                       for a, b in zip(first, second)]
        self.sizes = ref.cell_sizes(self.levels, LO, HI)
        plotfile.write_plotfile(self.path, NAMES, self.levels, LO, HI, RATIO)

    @functools.lru_cache(maxsize=None)
    def grid(self, name, level, lo, dims, min_level=0, fill=math.nan):
        return cg.covering_grid(self.levels, RATIO, NAMES.index(name), level, lo, dims, fill,
                                min_level)

    @functools.lru_cache(maxsize=None)
    def split(self, level, lo, dims, min_level=0, fill=math.nan):
        """(solenoidal, compressive) spectra of the reference, of the reference's grids."""
        f = [fr.fft3d(self.grid(name, level, lo, dims, min_level, fill)["values"])
             for name in VELOCITY]
        return sr.helmholtz(*f, spectra.inverse_length(dims, self.sizes[level]))

    def check(self, got, level, lo, dims, edges=None, grids=True, min_level=0, fill=math.nan):
        """api.helmholtz's dict against the covering grids, then the transforms, the split, the
        bins and the inverses of the references."""
        size = self.sizes[level]
        edges = spectra.default_edges(dims, size) if edges is None else np.asarray(edges)
        assert got["level"] == level and got["lo"] == lo and got["dims"] == dims
        assert got["cell_size"] == size
        assert ref.same_bits(got["k_edges"], edges)
        assert ref.same_bits(got["k"], 0.5 * (edges[:-1] + edges[1:]))
        coverage = self.grid("vx", level, lo, dims, min_level, fill)["coverage"]
        assert got["absent"] == int((coverage == 0.0).sum())
        g, edges_sq = spectra.inverse_length_sq(dims, size), spectra.squared_edges(edges)
        cells = dims[0] * dims[1] * dims[2]
        outside = nonfinite = 0
        imag_max = 0.0
        for part, three in zip(("solenoidal", "compressive"), self.split(level, lo, dims,
                                                                          min_level, fill)):
            sums = got["power"][part] * float(cells) ** 2          # exact: a power of two
            counts = check_bins(got["modes"][part], sums, three, g, edges_sq)
            assert ref.same_bits(got["spectrum"][part], got["power"][part] / np.diff(edges))
            outside, nonfinite = outside + counts[0], nonfinite + counts[1]
            if grids:
                assert list(got[part]) == VELOCITY
                for name, spectrum in zip(VELOCITY, three):
                    real, imag = sr.ifft3d(spectrum)
                    assert len(differing(got[part][name], real)) == 0, (part, name)
                    imag_max = max(imag_max, float(np.abs(imag).max()))
            else:
                assert part not in got
        assert (got["outside"], got["nonfinite"]) == (outside, nonfinite)
        for key in ("power", "spectrum"):
            assert ref.same_bits(got[key]["total"], got[key]["solenoidal"] + got[key]["compressive"])
        fraction = spectra.compressive_fraction(got["power"]["solenoidal"],
                                                got["power"]["compressive"], edges)
        assert got["compressive_fraction"] == fraction and 0.0 < fraction < 1.0
        if grids:
            print("imag_max:", got["imag_max"], "the grids' largest:",
                  max(np.abs(a).max() for a in got["solenoidal"].values()))
            assert got["imag_max"] == imag_max
            assert imag_max <= 32.0 * math.log2(cells) * EPS * math.sqrt(sum(
                float((self.grid(name, level, lo, dims, min_level, fill)["values"] ** 2).sum())
                for name in VELOCITY))
        else:
            assert "imag_max" not in got


def check_bins(modes, sums, three, g, edges_sq):
    """test_power_spectrum_gpu.check_bins' rule for bins that three spectra were added into: the
    counts equal, the sums within (n_b - 1 + 1) 2^-53 sum p of math.fsum -- n_b - 1 roundings of
    the additions in any order, one of the reference.  Returns (outside, nonfinite)."""
    found = [fr.shell_sums(spectrum, g, edges_sq) for spectrum in three]
    want_modes = sum(one[0] for one in found)
    assert modes.dtype == np.int64 and np.array_equal(modes, want_modes)
    for b in range(len(want_modes)):
        p = [term for one in found for term in one[1][b]]
        total = math.fsum(p)
        bound = (max(len(p) - 1, 0) + 1) * EPS * total
        assert abs(sums[b] - total) <= bound, (b, len(p), sums[b], total, bound)
    return sum(one[2] for one in found), sum(one[3] for one in found)


@pytest.fixture(scope="module")
def plot(tmp_path_factory):
    return Plot(tmp_path_factory.mktemp("spectral") / "plt")


def test_api_helmholtz_on_both_levels_and_its_file(ctx, plot, tmp_path):
    whole0, whole1 = ((0, 0, 0), (16, 8, 8)), ((0, 0, 0), (32, 16, 16))
    out = str(tmp_path / "split.npz")
    got = api.helmholtz(plot.path, VELOCITY, level=0, output=out)
    plot.check(got, 0, *whole0)
    assert got["outside"] > 0 and got["nonfinite"] == 0 and got["absent"] == 0
    # the two parts add up to the field: the split's eight roundings and a round trip of 2^10
    # cells, on the norm of the three components (every one enters each part)
    norm = math.sqrt(sum(float((plot.grid(name, 0, *whole0)["values"] ** 2).sum())
                         for name in VELOCITY))
    for name in VELOCITY:
        values = plot.grid(name, 0, *whole0)["values"]
        back = got["solenoidal"][name] + got["compressive"][name]
        assert np.linalg.norm((back - values).ravel()) <= (32.0 * 10 + 8.0) * EPS * norm
    back = spectra.load_helmholtz_npz(out)
    assert set(back) == set(got)
    for key in ("level", "lo", "dims", "cell_size", "outside", "nonfinite", "absent",
                "compressive_fraction", "imag_max"):
        assert back[key] == got[key], key
    for key in ("power", "spectrum", "modes", "solenoidal", "compressive"):
        assert list(back[key]) == list(got[key])
        for name in got[key]:
            assert np.array_equal(back[key][name], got[key][name]), (key, name)
    # the default level is the finest loaded one
    finest = api.helmholtz(plot.path, VELOCITY, bins=6, k_range=(0.0, 40.0))
    plot.check(finest, 1, *whole1, edges=np.linspace(0.0, 40.0, 7))


def test_api_helmholtz_of_a_sub_region_and_without_grids(ctx, plot):
    region = ((4, 2, 2), (11, 5, 5))                   # 8 x 4 x 4 cells of level 1, across the patch
    size = plot.sizes[1]
    left = tuple(LO[a] + region[0][a] * size[a] for a in range(3))
    right = tuple(LO[a] + (region[1][a] + 1) * size[a] for a in range(3))
    by_index = api.helmholtz(plot.path, VELOCITY, level=1, region=region)
    by_edges = api.helmholtz(plot.path, VELOCITY, level=1, left_edge=left, right_edge=right)
    for got in (by_index, by_edges):
        plot.check(got, 1, region[0], (8, 4, 4))
    for part in ("solenoidal", "compressive"):
        for name in VELOCITY:
            assert len(differing(by_index[part][name], by_edges[part][name])) == 0
    bare = api.helmholtz(plot.path, VELOCITY, level=0, grids=False)
    plot.check(bare, 0, (0, 0, 0), (16, 8, 8), grids=False)


def test_cells_without_data_need_a_fill_value(ctx, plot):
    whole1 = ((0, 0, 0), (32, 16, 16))
    with pytest.raises(ValueError, match="hold no data"):
        api.helmholtz(plot.path, VELOCITY, level=1, min_level=1)
    with pytest.raises(ValueError, match="hold no data"):
        api.potential(plot.path, "rho", level=1, min_level=1)
    got = api.helmholtz(plot.path, VELOCITY, level=1, min_level=1, fill=0.0, grids=False)
    assert got["absent"] == 32 * 16 * 16 - 8 * 8 * 8
    plot.check(got, 1, *whole1, grids=False, min_level=1, fill=0.0)
    phi = api.potential(plot.path, "rho", level=1, min_level=1, fill=0.0)
    assert phi["absent"] == got["absent"]
    check_potential(plot, phi, "rho", 1.0, 1, *whole1, min_level=1, fill=0.0)


def check_potential(plot, got, name, constant, level, lo, dims, min_level=0, fill=math.nan):
    size = plot.sizes[level]
    assert got["level"] == level and got["lo"] == lo and got["dims"] == dims
    assert got["cell_size"] == size and got["constant"] == constant
    rho = plot.grid(name, level, lo, dims, min_level, fill)["values"]
    scale = -(constant / (4.0 * math.pi * math.pi))
    spectrum = sr.inverse_laplacian(fr.fft3d(rho), spectra.inverse_length_sq(dims, size), scale)
    real, imag = sr.ifft3d(spectrum)
    assert len(differing(got["potential"], real)) == 0
    assert got["imag_max"] == float(np.abs(imag).max())
    assert got["imag_max"] <= 32.0 * math.log2(rho.size) * EPS * np.linalg.norm(real.ravel())


def test_api_potential_by_bits_and_its_file(ctx, plot, tmp_path):
    out = str(tmp_path / "potential.npz")
    got = api.potential(plot.path, "rho", constant=-2.5, level=0, output=out)
    check_potential(plot, got, "rho", -2.5, 0, (0, 0, 0), (16, 8, 8))
    assert got["absent"] == 0 and got["potential"].any()
    back = spectra.load_potential_npz(out)
    assert set(back) == set(got) and np.array_equal(back["potential"], got["potential"])
    for key in ("level", "lo", "dims", "cell_size", "constant", "imag_max", "absent"):
        assert back[key] == got[key], key
    # the defaults: the first variable at the finest loaded level, constant 1; and a sub-region
    finest = api.potential(plot.path)
    check_potential(plot, finest, "vx", 1.0, 1, (0, 0, 0), (32, 16, 16))
    part = api.potential(plot.path, "rho", level=1, region=((4, 2, 2), (11, 5, 5)))
    check_potential(plot, part, "rho", 1.0, 1, (4, 2, 2), (8, 4, 4))


# ---- the C ABI -------------------------------------------------------------------------------------

def test_wrong_arguments_are_refused_and_the_arrays_untouched(ctx):
    shape, dims = (4, 8, 16), (16, 8, 4)
    spectrum = torch.full(shape + (2,), 0.5, dtype=torch.float64, device=ctx.device)
    values = torch.full(shape, 0.25, dtype=torch.float64, device=ctx.device)
    imag = torch.full(shape, 0.125, dtype=torch.float64, device=ctx.device)
    six = [torch.full(shape + (2,), float(i + 2), dtype=torch.float64, device=ctx.device)
           for i in range(6)]
    pointer = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    ints = lambda a: (None if a is None else
                      np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32)))
    doubles = lambda a: (None if a is None else
                         np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double)))
    three = lambda a: (None if a is None else
                       (C.c_void_p * 3)(*(t.data_ptr() if t is not None else None for t in a)))

    def untouched():
        ctx.synchronize()
        return bool((spectrum == 0.5).all()) and bool((values == 0.25).all()) and \
            bool((imag == 0.125).all()) and \
            all(bool((t == float(i + 2)).all()) for i, t in enumerate(six))

    def ifft(spectrum=spectrum, dims=dims, values=values, imag=imag):
        return _capi.lib().avr_field_ifft(ctx._handle, pointer(spectrum), ints(dims),
                                          pointer(values), pointer(imag))

    def split(spectra=six[:3], dims=dims, h=(1.0, 0.5, 2.0), compressive=six[3:]):
        return _capi.lib().avr_spectrum_helmholtz(ctx._handle, three(spectra), ints(dims),
                                                  doubles(h), three(compressive))

    def laplacian(spectrum=spectrum, dims=dims, g=(1.0, 0.25, 4.0), scale=1.0):
        return _capi.lib().avr_spectrum_inverse_laplacian(ctx._handle, pointer(spectrum),
                                                          ints(dims), doubles(g), scale)

    dims_message = "dims must be powers of two in [1, 1024]"
    overlap, six_overlap = "the spectrum, values and imag overlap", "two of the six spectra overlap"
    positive = "inverse_length must be finite and positive"
    flat = lambda t, at: t.view(-1)[at:]
    wrong = [
        (ifft, dict(spectrum=None), "null argument"),
        (ifft, dict(values=None), "null argument"),
        (ifft, dict(dims=None), "null argument"),
        (ifft, dict(dims=(16, 8, 3)), dims_message),
        (ifft, dict(dims=(2048, 8, 4)), dims_message),
        (ifft, dict(dims=(16, 0, 4)), dims_message),
        (ifft, dict(dims=(16, 8, 3), values=spectrum), dims_message),     # the dims win
        (ifft, dict(values=spectrum), overlap),
        (ifft, dict(values=flat(spectrum, 511), dims=(16, 8, 2)), overlap),
        (ifft, dict(imag=values), overlap),
        (ifft, dict(imag=flat(values, 255), dims=(16, 8, 2)), overlap),
        (ifft, dict(imag=flat(spectrum, 511), dims=(16, 8, 2)), overlap),
        (split, dict(spectra=None), "null argument"),
        (split, dict(compressive=None), "null argument"),
        (split, dict(h=None), "null argument"),
        (split, dict(spectra=[six[0], None, six[2]]), "null argument"),
        (split, dict(compressive=[six[3], six[4], None], dims=(16, 8, 3)), "null argument"),
        (split, dict(dims=(16, 8, 12), h=(0.0, 1.0, 1.0)), dims_message),
        (split, dict(h=(1.0, 0.0, 1.0)), positive),
        (split, dict(h=(1.0, 1.0, math.nan)), positive),
        (split, dict(h=(-1.0, 1.0, 1.0), compressive=six[:3]), positive),
        (split, dict(h=(1e-160, 1.0, 1.0)), "inverse_length is too small: its square underflows"),
        (split, dict(h=(1.0, 1.0, 1e153)),
         "inverse_length is too large: a squared wave number overflows"),
        (split, dict(compressive=six[:3]), six_overlap),
        (split, dict(spectra=[six[0], six[0], six[2]]), six_overlap),
        (split, dict(compressive=[six[3], six[4], flat(six[2], 511)], dims=(16, 8, 2)),
         six_overlap),
        (laplacian, dict(spectrum=None), "null argument"),
        (laplacian, dict(g=None), "null argument"),
        (laplacian, dict(dims=(16, 8, 5)), dims_message),
        (laplacian, dict(g=(1.0, 0.0, 1.0)), "inverse_length_sq must be finite and positive"),
        (laplacian, dict(g=(1.0, 1.0, math.inf), scale=math.nan),
         "inverse_length_sq must be finite and positive"),
        (laplacian, dict(scale=math.inf), "scale must be finite"),
        (laplacian, dict(scale=math.nan), "scale must be finite"),
    ]
    for call, arguments, message in wrong:
        assert call(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert _capi.lib().avr_last_error().decode() == message, arguments
        assert untouched(), arguments
    # ... and the calls that are in order write everything, imag only where it is asked for
    f = spectra_of(shape)

    def fill(tensor, array):
        tensor.copy_(on_device(ctx, array))
        ctx.join()                      # the library's stream behind torch's copy

    fill(spectrum, f[0])
    assert ifft(imag=None) == 0
    ctx.synchronize()
    assert len(differing(values.cpu().numpy(), inverse_of(shape)[0])) == 0
    assert bool((imag == 0.125).all())
    fill(spectrum, f[0])
    assert ifft() == 0
    ctx.synchronize()
    assert len(differing(imag.cpu().numpy(), inverse_of(shape)[1])) == 0
    for d in range(3):
        fill(six[d], f[d])
    assert split() == 0
    ctx.synchronize()
    want = sr.helmholtz(*f, (1.0, 0.5, 2.0))
    for d in range(3):
        assert len(differing(six[d].cpu().numpy(), want[0][d])) == 0
        assert len(differing(six[3 + d].cpu().numpy(), want[1][d])) == 0
    fill(spectrum, f[1])
    assert laplacian(scale=-0.5) == 0
    ctx.synchronize()
    assert len(differing(spectrum.cpu().numpy(),
                         sr.inverse_laplacian(f[1], (1.0, 0.25, 4.0), -0.5))) == 0
