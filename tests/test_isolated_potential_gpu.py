"""The isolated potential on the GPU: isolated_green_kernel and spectrum_multiply_kernel through
avr_isolated_green and avr_spectrum_multiply, Context.isolated_green and
Context.spectrum_multiply, api.isolated_potential_scene and api.isolated_potential, against the
numpy restatement of the definition (isolated_reference) on the covering grids of
covering_grid_reference.  Everything is equal by bits (a NaN equal to a NaN of any payload)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, plotfile, spectra

import covering_grid_reference as cg
import gradient_reference as ref
import isolated_reference as ir

pytestmark = pytest.mark.gpu
# (Px, Py, Pz): one cell, a partial trip, a flat grid, every axis different, a second workgroup
# (16384 cells each), the longest axis in the middle
PADDED = [(1, 1, 1), (4, 1, 1), (8, 4, 1), (16, 4, 8), (32, 32, 32), (4, 1024, 4)]
SIZE = (0.5, 0.25, 1.0)          # (dx, dy, dz)


def on_device(ctx, array):
    return torch.from_numpy(np.ascontiguousarray(array)).to(ctx.device)


def differing(got, want):
    return np.argwhere(np.ascontiguousarray(got).view(np.uint64) !=
                       np.ascontiguousarray(want).view(np.uint64))


# ---- 1. the Green's grid ---------------------------------------------------------------------------

@pytest.mark.parametrize("padded", PADDED)
def test_isolated_green_equals_the_reference_by_bits(ctx, padded):
    for scale, self_value in ((-0.3, 0.0), (2.5 / (4.0 * math.pi), 0.0), (-0.3, -1.428),
                              (0.7, 3.0)):
        got = ctx.isolated_green(padded, SIZE, scale, self_value)
        ctx.synchronize()
        assert got.shape == padded[::-1] and got.dtype == torch.float64 and got.is_contiguous()
        different = differing(got.cpu().numpy(), ir.green(padded, SIZE, scale, self_value))
        print(padded, scale, self_value, "differing cells:", len(different),
              different[:4].tolist())
        assert len(different) == 0
    default = ctx.isolated_green(padded, SIZE, -0.3)
    ctx.synchronize()
    assert float(default[0, 0, 0]) == 0.0 and not bool(torch.signbit(default[0, 0, 0]))


def test_isolated_green_checks_its_arguments(ctx):
    for wrong in ((4, 4), (4, 4, 4, 4)):
        with pytest.raises(ValueError, match="three values"):
            ctx.isolated_green(wrong, SIZE, 1.0)
    with pytest.raises(ValueError, match="three values"):
        ctx.isolated_green((4, 4, 4), (1.0, 1.0), 1.0)
    for wrong in ((4, 12, 4), (2048, 4, 4), (4, 4, 0), (1 << 20, 1 << 20, 1 << 20)):
        with pytest.raises(ValueError, match="dims must be powers of two"):
            ctx.isolated_green(wrong, SIZE, 1.0)
    with pytest.raises(ValueError, match="cell_size must be finite and positive"):
        ctx.isolated_green((4, 4, 4), (1.0, 0.0, 1.0), 1.0)
    with pytest.raises(ValueError, match="scale and self_value must be finite"):
        ctx.isolated_green((4, 4, 4), SIZE, 1.0, math.inf)


# ---- 2. the product of two spectra -----------------------------------------------------------------

def random_spectrum(padded, seed):
    rng = np.random.default_rng(sum(padded) + seed)
    shape = padded[::-1] + (2,)
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 3.0, shape)


def multiplied(ctx, a, b):
    on_a, on_b = on_device(ctx, a), on_device(ctx, b)
    got = ctx.spectrum_multiply(on_a, on_b)
    ctx.synchronize()
    assert got.data_ptr() == on_a.data_ptr()                          # in place
    assert len(differing(on_b.cpu().numpy(), b)) == 0                 # b is only read
    return got.cpu().numpy()


@pytest.mark.parametrize("padded", PADDED)
def test_spectrum_multiply_equals_the_reference_by_bits(ctx, padded):
    a, b = random_spectrum(padded, 1), random_spectrum(padded, 2)
    different = differing(multiplied(ctx, a, b), ir.multiply(a, b))
    print(padded, "differing components:", len(different), different[:4].tolist())
    assert len(different) == 0


def test_spectrum_multiply_with_a_nan_mode_and_with_negative_zeros(ctx):
    padded = (16, 4, 8)
    a, b = random_spectrum(padded, 3), random_spectrum(padded, 4)
    a[3, 1, 5, 0] = math.nan
    b[7, 3, 15, 1] = math.inf
    got, want = multiplied(ctx, a, b), ir.multiply(a, b)
    assert ref.same_bits(got, want)
    assert np.isnan(want[3, 1, 5]).all() and np.isnan(want).sum() == 2
    assert np.isinf(want[7, 3, 15]).all()
    # signed zeros: the products' signs and (+0) + (-0) = +0 are IEEE's
    a, b = random_spectrum(padded, 5), random_spectrum(padded, 6)
    a[0, 0, :8] = [[-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0], [0.0, 0.0]] * 2
    b[0, 0, 4:8] = -np.abs(b[0, 0, 4:8])
    a[1, 0, :4] = [[-0.0, 1.0], [1.0, -0.0], [-0.0, -1.0], [-1.0, -0.0]]
    b[1, 0, :4] = [[-0.0, -0.0], [0.0, -0.0], [-0.0, 0.0], [-0.0, 2.0]]
    got, want = multiplied(ctx, a, b), ir.multiply(a, b)
    assert len(differing(got, want)) == 0
    assert np.signbit(want[:2, 0, :8]).any() and not np.signbit(want[:2, 0, :8]).all()


def test_spectrum_multiply_takes_two_spectra_of_one_shape(ctx):
    a = on_device(ctx, random_spectrum((16, 4, 8), 1))
    with pytest.raises(ValueError, match="one shape"):
        ctx.spectrum_multiply(a, on_device(ctx, random_spectrum((8, 4, 16), 1)))
    for wrong in (a.float(), a[:, :, ::2], a[..., 0], a.cpu()):
        with pytest.raises(ValueError):
            ctx.spectrum_multiply(a, wrong)
        with pytest.raises(ValueError):
            ctx.spectrum_multiply(wrong, a)
    with pytest.raises(ValueError, match="the two spectra overlap"):
        ctx.spectrum_multiply(a, a)


# ---- 3. the whole chain ----------------------------------------------------------------------------

DOMAINS = [((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))]
BOXES = [[((0, 0, 0), (15, 7, 7))], [((8, 4, 4), (15, 11, 11))]]
LO, HI, RATIO = (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [2]
NAMES = ["rho", "mass", "spoilt"]
NAN_AT = (1, 2, 3)                # (k, j, i) of level 0, outside the finer patch


class Plot:
    """A 16 x 8 x 8 plotfile with one finer patch and three fields: gradient_reference's normal
    field, its integer field, and the normal field with one NaN cell on level 0 (the cells under
    the patch hold 1e30 in all of them)."""

    def __init__(self, path):
        self.path = str(path)
        made = ref.make_levels(DOMAINS, BOXES, RATIO, 85)
        self.levels = []
        for l, level in enumerate(made):
            data = []
            for cells in level["data"]:
                spoilt = cells[0].copy()
                if l == 0:
                    spoilt[NAN_AT] = math.nan
                data.append(np.stack([cells[0], cells[2], spoilt]))
            self.levels.append({"domain": level["domain"], "boxes": level["boxes"], "data": data})
        self.sizes = ref.cell_sizes(self.levels, LO, HI)
        plotfile.write_plotfile(self.path, NAMES, self.levels, LO, HI, RATIO)

    @functools.lru_cache(maxsize=None)
    def grid(self, name, level, lo, dims, min_level=0, fill=math.nan):
        return cg.covering_grid(self.levels, RATIO, NAMES.index(name), level, lo, dims, fill,
                                min_level)

    @functools.lru_cache(maxsize=None)
    def potential(self, name, level, lo, dims, constant, self_term, min_level=0, fill=math.nan):
        rho = self.grid(name, level, lo, dims, min_level, fill)["values"]
        scale, self_value = ir.host_values(constant, self.sizes[level], self_term)
        return ir.isolated_potential(rho, self.sizes[level], scale, self_value)

    def check(self, got, name, level, lo, dims, constant=1.0, self_term=0.0, min_level=0,
              fill=math.nan):
        """api.isolated_potential's dict against the covering grid and then the convolution of
        the references."""
        assert got["level"] == level and got["lo"] == lo and got["dims"] == dims
        assert got["cell_size"] == self.sizes[level]
        assert got["constant"] == constant and got["self_term"] == self_term
        want = self.potential(name, level, lo, dims, constant, self_term, min_level, fill)
        assert got["padded_dims"] == want["padded_dims"] == spectra.padded_dims(dims)
        coverage = self.grid(name, level, lo, dims, min_level, fill)["coverage"]
        assert got["absent"] == int((coverage == 0.0).sum())
        assert got["potential"].shape == dims[::-1] and got["potential"].dtype == np.float64
        different = differing(got["potential"], want["potential"])
        print(name, level, lo, dims, "differing cells:", len(different), "imag_max",
              got["imag_max"], "of", float(np.abs(want["potential"]).max()))
        assert len(different) == 0
        assert got["imag_max"] == want["imag_max"]
        assert got["imag_max"] <= 100.0 * ir.unit(want)
        return want


@pytest.fixture(scope="module")
def plot(tmp_path_factory):
    return Plot(tmp_path_factory.mktemp("isolated") / "plt")


def test_api_isolated_potential_on_both_levels_and_its_file(ctx, plot, tmp_path):
    out = str(tmp_path / "isolated.npz")
    got = api.isolated_potential(plot.path, "rho", constant=-2.5, level=0, output=out)
    plot.check(got, "rho", 0, (0, 0, 0), (16, 8, 8), constant=-2.5)
    assert got["absent"] == 0 and got["potential"].any() and got["padded_dims"] == (32, 16, 16)
    back = spectra.load_isolated_potential_npz(out)
    assert set(back) == set(got) and np.array_equal(back["potential"], got["potential"])
    for key in ("level", "lo", "dims", "padded_dims", "cell_size", "constant", "self_term",
                "imag_max", "absent"):
        assert back[key] == got[key] and type(back[key]) is type(got[key]), key
    # the defaults: the first variable at the finest loaded level, constant 1, no self term
    finest = api.isolated_potential(plot.path)
    plot.check(finest, "rho", 1, (0, 0, 0), (32, 16, 16))
    assert finest["padded_dims"] == (64, 32, 32)


def test_api_isolated_potential_of_a_region_that_is_no_power_of_two(ctx, plot):
    region = ((4, 2, 2), (8, 8, 7))                    # 5 x 7 x 6 cells of level 1, across the patch
    size = plot.sizes[1]
    left = tuple(LO[a] + region[0][a] * size[a] for a in range(3))
    right = tuple(LO[a] + (region[1][a] + 1) * size[a] for a in range(3))
    by_index = api.isolated_potential(plot.path, "mass", level=1, region=region,
                                      constant=4.0 * math.pi)
    by_edges = api.isolated_potential(plot.path, "mass", level=1, left_edge=left,
                                      right_edge=right, constant=4.0 * math.pi)
    for got in (by_index, by_edges):
        plot.check(got, "mass", 1, region[0], (5, 7, 6), constant=4.0 * math.pi)
        assert got["padded_dims"] == (16, 16, 16) and got["absent"] == 0
    assert len(differing(by_index["potential"], by_edges["potential"])) == 0
    # a single line of cells and a single cell
    line = api.isolated_potential(plot.path, "rho", level=0, region=((2, 3, 1), (10, 3, 1)))
    plot.check(line, "rho", 0, (2, 3, 1), (9, 1, 1))
    one = api.isolated_potential(plot.path, "rho", level=0, region=((2, 3, 1), (2, 3, 1)),
                                 self_term=2.0)
    want = plot.check(one, "rho", 0, (2, 3, 1), (1, 1, 1), self_term=2.0)
    assert one["padded_dims"] == (1, 1, 1) and want["potential"].any()


def test_a_self_term_enters_the_potential(ctx, plot):
    region, dims = ((1, 0, 2), (5, 6, 7)), (5, 7, 6)
    self_term = 2.38 / plot.sizes[0][0]
    got = api.isolated_potential(plot.path, "rho", level=0, region=region, self_term=self_term)
    plot.check(got, "rho", 0, region[0], dims, self_term=self_term)
    bare = api.isolated_potential(plot.path, "rho", level=0, region=region)
    want = plot.check(bare, "rho", 0, region[0], dims)
    rho = plot.grid("rho", 0, region[0], dims)["values"]
    _, self_value = ir.host_values(1.0, plot.sizes[0], self_term)
    assert self_value != 0.0
    assert np.abs(got["potential"] - bare["potential"] - self_value * rho).max() <= \
        100.0 * ir.unit(plot.potential("rho", 0, region[0], dims, 1.0, self_term))
    assert want["potential"].any()


def test_cells_without_data_need_a_fill_value(ctx, plot):
    region, dims = ((6, 2, 2), (10, 8, 7)), (5, 7, 6)  # the patch begins at (8, 4, 4): 60 cells lie on it
    with pytest.raises(ValueError, match="hold no data"):
        api.isolated_potential(plot.path, "rho", level=1, region=region, min_level=1)
    got = api.isolated_potential(plot.path, "rho", level=1, region=region, min_level=1, fill=0.0)
    plot.check(got, "rho", 1, region[0], dims, min_level=1, fill=0.0)
    assert 0 < got["absent"] < 5 * 7 * 6
    filled = api.isolated_potential(plot.path, "rho", level=1, region=region, min_level=1,
                                    fill=-3.5)
    plot.check(filled, "rho", 1, region[0], dims, min_level=1, fill=-3.5)
    assert filled["absent"] == got["absent"]
    assert len(differing(filled["potential"], got["potential"])) > 0


def test_one_nan_cell_makes_the_whole_potential_nan(ctx, plot):
    region, dims = ((0, 0, 0), (4, 6, 5)), (5, 7, 6)
    got = api.isolated_potential(plot.path, "spoilt", level=0, region=region)
    want = plot.potential("spoilt", 0, region[0], dims, 1.0, 0.0)
    assert np.isnan(plot.grid("spoilt", 0, region[0], dims)["values"]).sum() == 1
    assert got["absent"] == 0 and got["potential"].shape == (6, 7, 5)
    assert ref.same_bits(got["potential"], want["potential"])
    assert np.isnan(got["potential"]).all() and math.isnan(got["imag_max"])
    assert math.isnan(want["imag_max"])


# ---- the C ABI -------------------------------------------------------------------------------------

def test_wrong_arguments_are_refused_and_the_arrays_untouched(ctx):
    padded, shape = (16, 8, 4), (4, 8, 16)
    green = torch.full(shape, 0.25, dtype=torch.float64, device=ctx.device)
    a = torch.full(shape + (2,), 0.5, dtype=torch.float64, device=ctx.device)
    b = torch.full(shape + (2,), 0.125, dtype=torch.float64, device=ctx.device)
    pointer = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    ints = lambda v: (None if v is None else
                      np.ascontiguousarray(v, np.int32).ctypes.data_as(C.POINTER(C.c_int32)))
    doubles = lambda v: (None if v is None else
                         np.ascontiguousarray(v, np.float64).ctypes.data_as(C.POINTER(C.c_double)))

    def untouched():
        ctx.synchronize()
        return bool((green == 0.25).all()) and bool((a == 0.5).all()) and \
            bool((b == 0.125).all())

    def make(dims=padded, size=SIZE, scale=-0.3, self_value=1.5, green=green):
        return _capi.lib().avr_isolated_green(ctx._handle, ints(dims), doubles(size), scale,
                                              self_value, pointer(green))

    def multiply(a=a, b=b, dims=padded):
        return _capi.lib().avr_spectrum_multiply(ctx._handle, pointer(a), pointer(b), ints(dims))

    dims_message = "dims must be powers of two in [1, 1024]"
    positive = "cell_size must be finite and positive"
    finite = "scale and self_value must be finite"
    overlap = "the two spectra overlap"
    flat = lambda t, at: t.view(-1)[at:]
    wrong = [
        (make, dict(dims=None), "null argument"),
        (make, dict(size=None), "null argument"),
        (make, dict(green=None), "null argument"),
        (make, dict(green=None, dims=(16, 8, 3)), "null argument"),
        (make, dict(dims=(16, 8, 3)), dims_message),
        (make, dict(dims=(2048, 8, 4)), dims_message),
        (make, dict(dims=(16, 0, 4)), dims_message),
        (make, dict(dims=(16, 12, 4), size=(0.0, 1.0, 1.0)), dims_message),   # the dims win
        (make, dict(size=(1.0, 0.0, 1.0)), positive),
        (make, dict(size=(1.0, 1.0, math.nan)), positive),
        (make, dict(size=(-1.0, 1.0, 1.0), scale=math.nan), positive),
        (make, dict(size=(math.inf, 1.0, 1.0)), positive),
        (make, dict(size=(1e-160, 1.0, 1.0)), "cell_size is too small: its square underflows"),
        (make, dict(size=(1.0, 1.0, 1e153)),
         "cell_size is too large: a squared distance overflows"),
        (make, dict(scale=math.inf), finite),
        (make, dict(scale=math.nan), finite),
        (make, dict(self_value=-math.inf), finite),
        (make, dict(self_value=math.nan), finite),
        (multiply, dict(a=None), "null argument"),
        (multiply, dict(b=None), "null argument"),
        (multiply, dict(dims=None), "null argument"),
        (multiply, dict(b=None, dims=(16, 8, 3)), "null argument"),
        (multiply, dict(dims=(16, 8, 3)), dims_message),
        (multiply, dict(dims=(2048, 8, 4)), dims_message),
        (multiply, dict(dims=(16, 8, 5), b=a), dims_message),                    # the dims win
        (multiply, dict(b=a), overlap),
        (multiply, dict(b=flat(a, 2), dims=(16, 8, 2)), overlap),
        (multiply, dict(b=flat(a, 511), dims=(16, 8, 2)), overlap),
        (multiply, dict(a=flat(b, 511), dims=(16, 8, 2)), overlap),
    ]
    for call, arguments, message in wrong:
        assert call(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert _capi.lib().avr_last_error().decode() == message, arguments
        assert untouched(), arguments
    # ... and the calls that are in order write everything; two halves of one array may be
    # multiplied, for they share no byte
    assert make() == 0
    ctx.synchronize()
    assert len(differing(green.cpu().numpy(), ir.green(padded, SIZE, -0.3, 1.5))) == 0
    first, second = random_spectrum(padded, 7), random_spectrum(padded, 8)
    a.copy_(on_device(ctx, first))
    b.copy_(on_device(ctx, second))
    ctx.join()                          # the library's stream behind torch's copies
    assert multiply() == 0
    ctx.synchronize()
    assert len(differing(a.cpu().numpy(), ir.multiply(first, second))) == 0
    assert len(differing(b.cpu().numpy(), second)) == 0
    b.copy_(on_device(ctx, second))
    ctx.join()
    assert multiply(a=b, b=flat(b, 512), dims=(16, 8, 2)) == 0
    ctx.synchronize()
    assert len(differing(b.cpu().numpy()[:2], ir.multiply(second[:2], second[2:]))) == 0
    assert len(differing(b.cpu().numpy()[2:], second[2:])) == 0
