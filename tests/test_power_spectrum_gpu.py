"""Power spectra on the GPU: the kernels of avr_fft.hip through avr_field_fft and
avr_spectrum_bins, Context.fft3d and Context.spectrum_bins, api.power_spectrum_scene and
api.power_spectrum, against the numpy restatement of the definitions (fft_reference).  The
transform is equal by bits; the bins' counts are equal and their sums lie within the a-priori bound
of adding non-negative terms in any order around a math.fsum reference."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, plotfile, spectra

import covering_grid_reference as cg
import derive_reference
import fft_reference as fr
import gradient_reference as ref

pytestmark = pytest.mark.gpu
VARIABLES = list(ref.VARIABLES)
EPS = 2.0 ** -53
# (nz, ny, nx): a length-1 axis, a line shorter than a wave, the longest line, both strided
# passes, odd and even log2, nx below the column group; the last two are the longest strided
# lines with a partial column group
SHAPES = [(1, 1, 1), (1, 1, 2), (2, 1, 4), (8, 4, 2), (4, 8, 16), (1, 2, 1024), (2, 1024, 2),
          (32, 32, 32), (1024, 1, 2), (1, 1024, 1)]
SIZE = (0.5, 0.25, 1.0)         # (dx, dy, dz) of the shell-sum cases


@pytest.fixture(autouse=True)
def _empty_registries():
    def clear():
        for name in list(api.derived_fields()):
            api.remove_field(name)
    clear()
    yield
    clear()


@functools.lru_cache(maxsize=None)
def case(shape):
    """(values, the reference's spectrum) of a shape, made once; treat both as read-only."""
    rng = np.random.default_rng(sum(shape))
    values = rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 3.0, shape)
    return values, fr.fft3d(values)


def on_device(ctx, array):
    return torch.from_numpy(np.ascontiguousarray(array)).to(ctx.device)


def check_bins(got, spectrum, g, edges_sq, before=None):
    """got = (modes, sums, totals or None) as numpy arrays against the reference's shell sums of
    `spectrum`; before: what the outputs held.  Returns the reference's (modes, per bin its
    terms, outside, nonfinite)."""
    modes, terms, outside, nonfinite = fr.shell_sums(spectrum, g, edges_sq)
    had_modes, had_sums, had_totals = before or (0, 0.0, np.zeros(2, dtype=np.int64))
    print("modes:", modes.tolist()[:12], "outside:", outside, "nonfinite:", nonfinite)
    assert got[0].dtype == np.int64 and np.array_equal(got[0] - had_modes, modes)
    if got[2] is not None:
        assert (got[2] - had_totals).tolist() == [outside, nonfinite]
    assert int(modes.sum()) + outside + nonfinite == spectrum[..., 0].size
    for b, p in enumerate(terms):
        total = math.fsum(p)
        had = float(np.broadcast_to(had_sums, modes.shape)[b])
        # (n_b - 1) roundings of the additions, one of the fsum reference -- and one more for
        # the addition to what the output held
        bound = (max(len(p) - 1, 0) + 1 + (1 if had else 0)) * EPS * (total + abs(had))
        assert abs(got[1][b] - had - total) <= bound, (b, len(p), got[1][b], total, bound)
    return modes, terms, outside, nonfinite


def bins_of(ctx, spectrum, g, edges_sq, out=None):
    found = ctx.spectrum_bins(on_device(ctx, spectrum), g, edges_sq, out)
    ctx.synchronize()
    return tuple(t.cpu().numpy() for t in found)


# ---- 1. table and transform ------------------------------------------------------------------------

def test_the_library_makes_the_twiddle_table_python_makes_by_bits(avr_lib):
    for p in range(1, 11):
        n = 1 << p
        table = np.full((n // 2, 2), -7.0)
        assert avr_lib.avr_fft_twiddles(n, table.ctypes.data_as(C.POINTER(C.c_double))) == 0
        assert ref.same_bits(table, fr.twiddles(n)), n


@pytest.mark.parametrize("shape", SHAPES)
def test_fft3d_equals_the_reference_by_bits(ctx, avr_lib, shape):
    for n in set(shape) - {1}:      # named for what it is, should the two libms ever differ
        table = np.zeros((n // 2, 2))
        assert avr_lib.avr_fft_twiddles(n, table.ctypes.data_as(C.POINTER(C.c_double))) == 0
        assert ref.same_bits(table, fr.twiddles(n)), n
    values, want = case(shape)
    spectrum = ctx.fft3d(on_device(ctx, values))
    ctx.synchronize()
    got = spectrum.cpu().numpy()
    assert got.shape == shape + (2,) and got.dtype == np.float64
    different = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
    print(shape, "differing components:", len(different), different[:4].tolist())
    assert len(different) == 0
    again = ctx.fft3d(on_device(ctx, values))
    ctx.synchronize()
    assert torch.equal(again.view(torch.int64), spectrum.view(torch.int64))


def test_a_field_of_small_integers_transforms_exactly(ctx):
    values = np.arange(8, dtype=np.float64).reshape(2, 2, 2) - 3.0
    got = ctx.fft3d(on_device(ctx, values))
    ctx.synchronize()
    want = np.fft.fftn(values)
    assert np.array_equal(got.cpu().numpy()[..., 0], want.real)
    assert np.array_equal(got.cpu().numpy()[..., 1], want.imag)


def test_fft3d_takes_contiguous_float64_grids_only(ctx):
    values = on_device(ctx, case((4, 8, 16))[0])
    for wrong in (values.float(), values[:, :, ::2], values[0], values.cpu()):
        with pytest.raises(ValueError):
            ctx.fft3d(wrong)
    for shape in ((4, 8, 12), (4, 8, 2048)):
        with pytest.raises(ValueError, match="dims must be powers of two"):
            ctx.fft3d(torch.zeros(shape, dtype=torch.float64, device=ctx.device))


# ---- 2. shell sums ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_default_edges_on_every_shape(ctx, shape):
    dims = shape[::-1]
    edges = spectra.default_edges(dims, SIZE)
    g, edges_sq = spectra.inverse_length_sq(dims, SIZE), spectra.squared_edges(edges)
    check_bins(bins_of(ctx, case(shape)[1], g, edges_sq), case(shape)[1], g, edges_sq)


def test_the_integer_field_sums_by_bits(ctx):
    values = np.arange(8, dtype=np.float64).reshape(2, 2, 2) - 3.0
    spectrum = fr.fft3d(values)
    g = spectra.inverse_length_sq((2, 2, 2), (1.0, 1.0, 1.0))
    edges_sq = spectra.squared_edges([0.0, 1.0, 4.0, 5.0, 6.0])
    got = bins_of(ctx, spectrum, g, edges_sq)
    modes, terms, _, _ = check_bins(got, spectrum, g, edges_sq)
    assert modes.tolist() == [1, 3, 3, 1] and got[2].tolist() == [0, 0]
    assert ref.same_bits(got[1], [math.fsum(p) for p in terms])
    assert got[1].sum() == 8.0 * float((values ** 2).sum())         # Parseval, exactly


def test_logarithmic_and_explicit_edges_and_a_k_range_that_cuts_the_modes(ctx):
    shape = (4, 8, 16)
    dims, spectrum = shape[::-1], case(shape)[1]
    g = spectra.inverse_length_sq(dims, SIZE)
    default = spectra.default_edges(dims, SIZE)
    log = spectra.make_edges(dims, SIZE, bins=7, k_log=True)
    cut = spectra.make_edges(dims, SIZE, bins=5, k_range=(default[2], default[3]))
    explicit = np.array([0.1, 1.0, 1.5, 9.0, 40.0])
    for edges in (log, cut, explicit):
        edges_sq = spectra.squared_edges(edges)
        got = bins_of(ctx, spectrum, g, edges_sq)
        modes, _, outside, _ = check_bins(got, spectrum, g, edges_sq)
        assert outside > 0 and modes.sum() > 0                        # some in, some cut


def test_one_bin_and_2048_bins(ctx):
    shape = (32, 32, 32)
    dims, spectrum = shape[::-1], case(shape)[1]
    g = spectra.inverse_length_sq(dims, SIZE)
    k_max = 2.0 * math.pi * math.sqrt(sum((0.5 / s) ** 2 for s in SIZE))
    for edges in (np.array([0.0, 2.0 * k_max]), np.linspace(0.0, 0.75 * k_max, 2049)):
        edges_sq = spectra.squared_edges(edges)
        got = bins_of(ctx, spectrum, g, edges_sq)
        modes, _, outside, _ = check_bins(got, spectrum, g, edges_sq)
        assert got[0].shape == (edges.size - 1,)
    assert np.count_nonzero(modes) > 100 and outside > 0    # of the 2048: many bins, and a cut


def test_modes_on_the_edges_land_where_the_rule_says(ctx):
    spectrum = np.ones((1, 1, 4, 2))
    g = spectra.inverse_length_sq((4, 1, 1), (0.25, 1.0, 1.0))      # q = 0, 1, 4, 1
    for edges_sq, modes, outside in (([0.0, 1.0, 4.0], [1, 3], 0), ([1.0, 4.0], [3], 1),
                                     ([0.0, 0.5, 1.0], [1, 2], 1)):
        got = bins_of(ctx, spectrum, g, np.array(edges_sq))
        assert got[0].tolist() == modes and got[2].tolist() == [outside, 0]
        assert got[1].tolist() == [2.0 * m for m in modes]


def test_outputs_that_already_hold_values_are_added_to(ctx):
    shape = (8, 4, 2)
    dims, spectrum = shape[::-1], case(shape)[1]
    edges = spectra.default_edges(dims, SIZE)
    g, edges_sq = spectra.inverse_length_sq(dims, SIZE), spectra.squared_edges(edges)
    n = edges.size - 1
    had = (np.arange(n, dtype=np.int64) + 5, np.linspace(1.0, 2.0, n),
           np.array([7, 9], dtype=np.int64))
    out = tuple(on_device(ctx, a.copy()) for a in had)
    found = ctx.spectrum_bins(on_device(ctx, spectrum), g, edges_sq, out)
    ctx.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(found, out))
    check_bins(tuple(t.cpu().numpy() for t in out), spectrum, g, edges_sq, before=had)
    with pytest.raises(ValueError):
        ctx.spectrum_bins(on_device(ctx, spectrum), g, edges_sq, (out[0], out[1][:1], out[2]))
    ctx.synchronize()


def test_one_nan_cell_makes_every_mode_nonfinite(ctx):
    values = case((4, 8, 16))[0][:, :4, :4].copy()
    values[1, 2, 3] = math.nan
    g = spectra.inverse_length_sq((4, 4, 4), SIZE)
    edges_sq = spectra.squared_edges(spectra.default_edges((4, 4, 4), SIZE))
    modes, sums, totals = ctx.spectrum_bins(ctx.fft3d(on_device(ctx, values)), g, edges_sq)
    ctx.synchronize()
    assert totals.tolist() == [0, 64] and not modes.any() and not sums.any()


# ---- 3. the API ------------------------------------------------------------------------------------

DOMAINS = [((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))]
BOXES = [[((0, 0, 0), (15, 7, 7))], [((8, 4, 4), (15, 11, 11))]]
LO, HI, RATIO = (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [2]


class Plot:
    def __init__(self, path):
        self.path = str(path)
        self.levels = ref.make_levels(DOMAINS, BOXES, RATIO, 81)
        self.sizes = ref.cell_sizes(self.levels, LO, HI)
        plotfile.write_plotfile(self.path, VARIABLES, self.levels, LO, HI, RATIO)
        squared = derive_reference.evaluate_levels("u * u", self.levels, VARIABLES, LO, HI)
        self.squared = [{"domain": lev["domain"], "boxes": lev["boxes"],
                         "data": [g[None] for g in grids_]}
                        for lev, grids_ in zip(self.levels, squared)]

    @functools.lru_cache(maxsize=None)
    def grid(self, name, level, lo, dims, min_level=0, fill=math.nan):
        levels, component = (self.squared, 0) if name == "uu" else (self.levels,
                                                                     VARIABLES.index(name))
        return cg.covering_grid(levels, RATIO, component, level, lo, dims, fill, min_level)

    def check(self, got, names, level, lo, dims, edges=None, min_level=0, fill=math.nan):
        """api.power_spectrum's dict against the covering grid, then the transform, then the
        bins of the references."""
        size = self.sizes[level]
        edges = spectra.default_edges(dims, size) if edges is None else np.asarray(edges)
        assert got["level"] == level and got["lo"] == lo and got["dims"] == dims
        assert got["cell_size"] == size and list(got["fields"]) == list(names)
        assert ref.same_bits(got["k_edges"], edges)
        assert ref.same_bits(got["k"], 0.5 * (edges[:-1] + edges[1:]))
        g, edges_sq = spectra.inverse_length_sq(dims, size), spectra.squared_edges(edges)
        cells = dims[0] * dims[1] * dims[2]
        total, outside, nonfinite = 0.0, 0, 0
        for name in names:
            grid = self.grid(name, level, lo, dims, min_level, fill)
            assert got["absent"] == int((grid["coverage"] == 0.0).sum())
            one = got["fields"][name]
            sums = one["power"] * float(cells) ** 2          # exact: a power of two
            counts = check_bins((one["modes"], sums, None), fr.fft3d(grid["values"]), g, edges_sq)
            assert ref.same_bits(one["spectrum"], one["power"] / np.diff(edges))
            outside, nonfinite = outside + counts[2], nonfinite + counts[3]
            total = total + one["power"]
        assert ref.same_bits(got["total"], total)
        assert (got["outside"], got["nonfinite"]) == (outside, nonfinite)


@pytest.fixture(scope="module")
def plot(tmp_path_factory):
    return Plot(tmp_path_factory.mktemp("spectrum") / "plt")


def test_api_power_spectrum_of_stored_and_derived_fields_on_both_levels(ctx, plot, tmp_path):
    whole0, whole1 = ((0, 0, 0), (16, 8, 8)), ((0, 0, 0), (32, 16, 16))
    out = str(tmp_path / "spectrum.npz")
    got = api.power_spectrum(plot.path, ["u"], level=0, output=out)
    plot.check(got, ["u"], 0, *whole0)
    assert got["outside"] > 0 and got["nonfinite"] == 0 and got["absent"] == 0
    assert got["fields"]["u"]["modes"].tolist()[:2] == [1, 2]      # L = (2, 1, 1): mx = +-1
    mean_square = float((plot.grid("u", 0, *whole0)["values"] ** 2).mean())
    everything = api.power_spectrum(plot.path, ["u"], level=0, edges=[0.0, 1e3])
    assert everything["outside"] == 0
    assert abs(everything["total"][0] - mean_square) <= 64 * 10 * EPS * mean_square  # Parseval

    back = spectra.load_npz(out)
    assert set(back) == set(got) and list(back["fields"]) == ["u"]
    for key in ("level", "lo", "dims", "cell_size", "outside", "nonfinite", "absent"):
        assert back[key] == got[key], key
    for key in ("k_edges", "k", "total"):
        assert ref.same_bits(back[key], got[key]), key
    for key in ("power", "spectrum", "modes"):
        assert np.array_equal(back["fields"]["u"][key], got["fields"]["u"][key])

    # the defaults: the first variable at the finest loaded level
    finest = api.power_spectrum(plot.path)
    plot.check(finest, ["u"], 1, *whole1)
    coarse = api.power_spectrum(plot.path, max_level=0)
    assert coarse["level"] == 0 and coarse["dims"] == (16, 8, 8)

    # a derived field, and three components in the order given
    api.add_field("uu", "u * u")
    names = ["whole", "uu", "u"]
    three = api.power_spectrum(plot.path, names, level=1, bins=6, k_range=(0.0, 40.0))
    plot.check(three, names, 1, *whole1, edges=np.linspace(0.0, 40.0, 7))
    parts = [three["fields"][name]["power"] for name in names]
    assert ref.same_bits(three["total"], (parts[0] + parts[1]) + parts[2])

    # a field with NaN and infinities: every mode is counted as not finite
    odd = api.power_spectrum(plot.path, ["odd"], level=0)
    assert odd["nonfinite"] == 16 * 8 * 8 and odd["outside"] == 0
    assert not odd["fields"]["odd"]["modes"].any() and not odd["total"].any()


def test_api_power_spectrum_of_a_sub_region_by_index_and_by_edges(ctx, plot):
    region = ((4, 2, 2), (11, 5, 5))                   # 8 x 4 x 4 cells of level 1, across the patch
    size = plot.sizes[1]
    left = tuple(LO[a] + region[0][a] * size[a] for a in range(3))
    right = tuple(LO[a] + (region[1][a] + 1) * size[a] for a in range(3))
    log = dict(bins=4, k_log=True)
    by_index = api.power_spectrum(plot.path, ["u"], level=1, region=region, **log)
    by_edges = api.power_spectrum(plot.path, ["u"], level=1, left_edge=left, right_edge=right,
                                  **log)
    edges = spectra.make_edges((8, 4, 4), size, **log)
    for got in (by_index, by_edges):
        plot.check(got, ["u"], 1, region[0], (8, 4, 4), edges=edges)
    for key in ("power", "spectrum", "modes"):
        assert np.array_equal(by_index["fields"]["u"][key], by_edges["fields"]["u"][key])


def test_cells_without_data_need_a_fill_value(ctx, plot):
    whole1 = ((0, 0, 0), (32, 16, 16))
    with pytest.raises(ValueError, match="hold no data"):
        api.power_spectrum(plot.path, ["u"], level=1, min_level=1)
    got = api.power_spectrum(plot.path, ["u"], level=1, min_level=1, fill=0.0)
    assert got["absent"] == 32 * 16 * 16 - 8 * 8 * 8
    plot.check(got, ["u"], 1, *whole1, min_level=1, fill=0.0)


# ---- the C ABI -------------------------------------------------------------------------------------

def test_wrong_arguments_are_refused_and_the_outputs_untouched(ctx):
    values = on_device(ctx, case((4, 8, 16))[0])
    spectrum = torch.full((4, 8, 16, 2), 0.5, dtype=torch.float64, device=ctx.device)
    modes = torch.full((3,), 7, dtype=torch.int64, device=ctx.device)
    power = torch.full((3,), 0.25, dtype=torch.float64, device=ctx.device)
    totals = torch.full((2,), 9, dtype=torch.int64, device=ctx.device)
    pointer = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    ints = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    doubles = lambda a: (None if a is None else
                         np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double)))

    def untouched():
        ctx.synchronize()
        return bool((spectrum == 0.5).all()) and bool((modes == 7).all()) and \
            bool((power == 0.25).all()) and bool((totals == 9).all())

    def fft(values=values, dims=(16, 8, 4), out=spectrum):
        return _capi.lib().avr_field_fft(ctx._handle, pointer(values), ints(dims), pointer(out))

    def bins(source=values, dims=(16, 8, 2), g=(1.0, 1.0, 1.0), edges=(0.0, 1.0, 2.0, 3.0), n=3,
             modes=modes, power=power, totals=totals):
        # `values` stands in for a spectrum of half as many modes: nothing the call may write
        return _capi.lib().avr_spectrum_bins(ctx._handle, pointer(source), ints(dims), doubles(g),
                                             doubles(edges), n, pointer(modes), pointer(power),
                                             pointer(totals))

    dims_message = "dims must be powers of two in [1, 1024]"
    wrong = [
        (fft, dict(values=None), "null argument"),
        (fft, dict(out=None), "null argument"),
        (fft, dict(dims=(16, 8, 3)), dims_message),
        (fft, dict(dims=(2048, 8, 4)), dims_message),
        (fft, dict(dims=(16, 0, 4)), dims_message),
        (fft, dict(values=spectrum), "the spectrum overlaps the input"),
        (fft, dict(values=spectrum.view(-1)[512:]), "the spectrum overlaps the input"),
        (bins, dict(source=None), "null argument"),
        (bins, dict(g=None), "null argument"),
        (bins, dict(edges=None), "null argument"),
        (bins, dict(modes=None), "null argument"),
        (bins, dict(power=None), "null argument"),
        (bins, dict(totals=None), "null argument"),
        (bins, dict(dims=(16, 8, 5)), dims_message),
        (bins, dict(n=0), "n_bins must lie in [1, 2048]"),
        (bins, dict(n=2049), "n_bins must lie in [1, 2048]"),
        (bins, dict(edges=(0.0, 1.0, math.inf, 3.0)), "edges_sq must be finite"),
        (bins, dict(edges=(-1.0, 1.0, 2.0, 3.0)), "edges_sq must not be negative"),
        (bins, dict(edges=(0.0, 1.0, 1.0, 3.0)), "edges_sq must be strictly increasing"),
        (bins, dict(g=(1.0, 0.0, 1.0)), "inverse_length_sq must be finite and positive"),
        (bins, dict(g=(1.0, 1.0, math.nan)), "inverse_length_sq must be finite and positive"),
        (bins, dict(source=power, dims=(1, 1, 1)), "an output array overlaps the spectrum"),
        (bins, dict(source=spectrum, power=spectrum.view(-1)[100:]),
         "an output array overlaps the spectrum"),
    ]
    for call, arguments, message in wrong:
        assert call(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert _capi.lib().avr_last_error().decode() == message, arguments
        assert untouched(), arguments
    # ... and the calls that are in order write everything
    assert fft() == 0
    ctx.synchronize()
    assert ref.same_bits(spectrum.cpu().numpy(), case((4, 8, 16))[1])
    assert bins(source=spectrum, dims=(16, 8, 4)) == 0
    ctx.synchronize()
    g, edges_sq = np.ones(3), np.array([0.0, 1.0, 2.0, 3.0])
    check_bins((modes.cpu().numpy(), power.cpu().numpy(), totals.cpu().numpy()),
               case((4, 8, 16))[1], g, edges_sq,
               before=(7, 0.25, np.array([9, 9], dtype=np.int64)))
