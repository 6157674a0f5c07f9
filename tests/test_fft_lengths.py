"""The transforms at the line lengths and group shapes they run at, without a GPU: the numpy
restatements (fft_reference.fft3d, spectral_reference.ifft3d) on lines of 64 to 1024 values in
each of the three passes, against the transform by its definition in long double
(fft_reference.exact_fft3d, exact_ifft3d) within the a-priori bound, on fields whose transform is
known exactly, and against the written-out line loops taken along the axes in the stated order.
tests/test_fft_lengths_gpu.py holds the kernels to the same shapes."""
import functools
import math

import numpy as np
import pytest

import fft_reference as fr
import gradient_reference as ref
import spectral_reference as sr

EPS = 2.0 ** -53
# (nz, ny, nx) by the length N of the longest line and the pass that takes it, chosen from the
# plan's constants (kFftGroupElements = 2048, kFftMinColumns = 4; tests/cxx/fft_plan_test.cpp
# holds the plan to what is said here, so a change of the constants asks for new shapes):
#   x: two full groups of 2048 / N whole lines (32, 16, 8, 4, 2 lines staged side by side)
#   y: two planes of two full groups of max(2048 / N, 4) columns
#   z: two full groups of max(2048 / N, 4) columns
# At N = 1024 a strided group is 4 columns: 4 x 1024 x 16 bytes, the 64 KiB a workgroup may ask
# for.
ROLES = {
    64: {"x": (1, 64, 64), "y": (2, 64, 64), "z": (64, 2, 32)},
    128: {"x": (1, 32, 128), "y": (2, 128, 32), "z": (128, 2, 16)},
    256: {"x": (1, 16, 256), "y": (2, 256, 16), "z": (256, 2, 8)},
    512: {"x": (1, 8, 512), "y": (2, 512, 8), "z": (512, 2, 4)},
    1024: {"x": (1, 4, 1024), "y": (2, 1024, 8), "z": (1024, 2, 4)},
}
CUBE = (64, 64, 64)             # the class of the timed grids (128^3 to 512^3): 128 groups a pass
SHAPES = [ROLES[n][role] for n in ROLES for role in "xyz"] + [CUBE]
FULL_LDS = [ROLES[1024]["y"], ROLES[1024]["z"]]         # the launches that stage 64 KiB
AXIS = {"x": 2, "y": 1, "z": 0}
# (shape, the axis of its long line) of the fields whose transform is known exactly
EXACT = [(ROLES[n][role], AXIS[role]) for n in (64, 512, 1024) for role in "xyz"]


def field(shape):
    """The transform tests' random values over six decades, seeded from the shape."""
    rng = np.random.default_rng(sum(shape))
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 3.0, shape)


@functools.lru_cache(maxsize=None)
def case(shape):
    """(values, the restatement's spectrum, the restatement's inverse of that spectrum as (real,
    imag)) of a shape, made once; treat them as read-only."""
    values = field(shape)
    spectrum = fr.fft3d(values)
    return values, spectrum, sr.ifft3d(spectrum)


def transform_bound(cells, norm):
    """16 log2(Ntot) 2^-53 ||.||: Higham's bound for Cooley-Tukey with the per-stage factor eta <~
    16 * 2^-53 of test_power_spectrum.test_the_reference_against_fftn_within_the_a_priori_bound,
    without that test's doubling for numpy.fft's own error: the long-double reference's is 2^-11
    of float64's.  A-priori, not measured."""
    return 16.0 * math.log2(cells) * EPS * norm


def norm2(*parts):
    """The 2-norm of all the parts together, accumulated in long double."""
    return float(np.sqrt(sum((np.asarray(p, dtype=np.longdouble) ** 2).sum() for p in parts)))


def exact_fields(shape, axis):
    """{name: (values, the spectrum [nz, ny, nx, 2] they transform to exactly)}: every product
    of the radix-2 stages is a table entry times a value whose sum holds no rounding, or a zero."""
    cells = float(np.prod(shape))
    delta = np.zeros(shape)
    delta[0, 0, 0] = 1.0
    ones = np.zeros(shape + (2,))
    ones[..., 0] = 1.0
    mean = np.zeros(shape + (2,))
    mean[0, 0, 0, 0] = -3.0 * cells
    where = [1, 1, 1]
    where[axis] = shape[axis]
    stripes = np.zeros(shape) + ((-1.0) ** np.arange(shape[axis])).reshape(where)
    nyquist = np.zeros(shape + (2,))
    at = [0, 0, 0]
    at[axis] = shape[axis] // 2
    nyquist[tuple(at) + (0,)] = cells
    return {"a unit delta at the origin": (delta, ones),
            "a constant": (np.full(shape, -3.0), mean),
            "alternating signs along the long line": (stripes, nyquist)}


# ---- the long-double reference itself --------------------------------------------------------------

def test_long_double_is_wider_than_float64_here():
    fr.require_long_double()
    assert abs(float(fr.long_pi() - np.longdouble(math.pi))) < 2.0 ** -52   # pi itself, not f64(pi)
    assert float(fr.long_pi()) == math.pi


def test_the_long_double_transform_on_answers_known_without_it():
    """The matrix, its index and the axes: a shifted delta against the closed form (which is a
    product of three phase vectors, no matrix), small integers exactly, and there and back."""
    shape, at = (2, 4, 8), (1, 3, 5)
    values = np.zeros(shape)
    values[at] = 0.125
    got = fr.exact_fft3d(values)
    want = fr.delta_spectrum(shape, at, 0.125)
    assert got[0].dtype == np.longdouble and got[0].shape == shape
    assert norm2(got[0] - want[0], got[1] - want[1]) <= 2.0 ** -60 * norm2(*want)
    # F[kz, ky, kx] of the delta by hand: 0.125 exp(-2 pi i (5 kx / 8 + 3 ky / 4 + kz / 2))
    assert abs(float(got[0][1, 0, 0]) + 0.125) <= 2.0 ** -60       # kz = 1: exp(-i pi) = -1
    assert abs(float(got[1][0, 1, 0]) - 0.125) <= 2.0 ** -60       # ky = 1: exp(-3 i pi / 2) = +i
    assert abs(float(got[0][0, 0, 1]) + 0.125 * math.sqrt(0.5)) <= 2.0 ** -55   # kx = 1: -5 pi / 4
    assert abs(float(got[1][0, 0, 1]) - 0.125 * math.sqrt(0.5)) <= 2.0 ** -55
    small = np.arange(8, dtype=np.float64).reshape(2, 2, 2) - 3.0
    re, im = fr.exact_fft3d(small)
    assert float(np.abs(re - fr.fft3d(small)[..., 0]).max()) <= 2.0 ** -58   # integers up to 12
    assert float(np.abs(im).max()) <= 2.0 ** -58
    rng = np.random.default_rng(3)
    re, im = rng.standard_normal(shape), rng.standard_normal(shape)
    forward = fr._dft_axes(re.astype(np.longdouble), im.astype(np.longdouble), 1)
    back = fr._dft_axes(*forward, -1)
    assert norm2(back[0] / 64 - re, back[1] / 64 - im) <= 2.0 ** -58 * norm2(re, im)
    # the mirror: one mode in, a plane wave out
    spectrum = np.zeros(shape + (2,))
    spectrum[at + (0,)] = 0.125
    got = fr.exact_ifft3d(spectrum[..., 0], spectrum[..., 1])
    want = fr.plane_wave(shape, at, 0.125)
    assert norm2(got[0] - want[0], got[1] - want[1]) <= 2.0 ** -60 * norm2(*want)
    assert abs(float(want[1][0, 1, 0]) + 0.125 / 64) <= 2.0 ** -66  # y = 1: exp(+3 i pi / 2) = -i


# ---- the restatements against it -------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_the_forward_restatement_against_the_long_double_transform(shape):
    values, spectrum, _ = case(shape)
    want = fr.exact_fft3d(values)
    error = norm2(spectrum[..., 0] - want[0], spectrum[..., 1] - want[1])
    norm = norm2(*want)
    bound = transform_bound(values.size, norm)
    print(shape, "error / (2^-53 norm):", error / (EPS * norm), "bound:", bound / (EPS * norm))
    assert spectrum.shape == shape + (2,) and norm > 0.0
    assert error <= bound


@pytest.mark.parametrize("shape", SHAPES)
def test_the_inverse_restatement_against_the_long_double_transform(shape):
    """The bound of test_spectral.test_the_inverse_against_ifftn_within_the_a_priori_bound without
    its doubling for numpy.fft's error."""
    _, spectrum, (real, imag) = case(shape)
    want = fr.exact_ifft3d(spectrum[..., 0], spectrum[..., 1])
    error = norm2(real - want[0], imag - want[1])
    norm = norm2(*want)
    bound = transform_bound(real.size, norm)
    print(shape, "error / (2^-53 norm):", error / (EPS * norm), "bound:", bound / (EPS * norm))
    assert real.shape == shape == imag.shape and norm > 0.0
    assert error <= bound


@pytest.mark.parametrize("shape, axis", EXACT)
def test_fields_whose_transform_is_known_exactly(shape, axis):
    for name, (values, want) in exact_fields(shape, axis).items():
        got = fr.fft3d(values)
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4].tolist())
    # ... and back: a spectrum of ones is the unit delta
    ones, delta = exact_fields(shape, axis)["a unit delta at the origin"][::-1]
    real, imag = sr.ifft3d(ones)
    assert np.array_equal(real, delta) and not imag.any()


def test_the_3d_restatements_are_the_line_loops_along_the_axes_in_the_stated_order():
    """fft3d is fft_line_loops along x, then y, then z, and ifft3d is line_loops along z, then y,
    then x, then the scale, by bits -- another order of the axes rounds differently."""
    shape = (2, 4, 64)
    values = field(shape)

    def along(axis, re, im, line):
        re, im = np.moveaxis(re, axis, -1).copy(), np.moveaxis(im, axis, -1).copy()
        for at in np.ndindex(re.shape[:-1]):
            re[at], im[at] = line(re[at], im[at])
        return np.moveaxis(re, -1, axis), np.moveaxis(im, -1, axis)

    re, im = values.copy(), np.zeros(shape)
    for axis in (2, 1, 0):
        re, im = along(axis, re, im, fr.fft_line_loops)
    spectrum = fr.fft3d(values)
    assert ref.same_bits(spectrum[..., 0], re) and ref.same_bits(spectrum[..., 1], im)
    for axis in (0, 1, 2):
        table = sr.inverse_twiddles(shape[axis])
        re, im = along(axis, re, im, lambda a, b: sr.line_loops(a, b, table))
    scale = 1.0 / float(values.size)
    real, imag = sr.ifft3d(spectrum)
    assert ref.same_bits(real, re * scale) and ref.same_bits(imag, im * scale)
