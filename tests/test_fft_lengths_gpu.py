"""The transform kernels at the line lengths and group shapes they run at: fft_x_kernel,
fft_column_kernel and ifft_x_kernel through Context.fft3d and Context.ifft3d on the sixteen grids
of test_fft_lengths.py -- lines of 64 to 1024 values in each pass, as many lines side by side in
LDS as the plan stages (32, 16, 8, 4), two groups a plane and two planes, and the two launches
that ask for all 64 KiB.  By bits against the numpy restatements; against closed forms in long
double that do not go through the restatements; exactly on fields whose transform holds no
rounding; there and back; and the isolated potential of a point mass on a padded line of 128."""
import math

import numpy as np
import pytest
import torch

import fft_reference as fr
import isolated_reference as ir
from test_fft_lengths import (CUBE, EPS, EXACT, FULL_LDS, ROLES, SHAPES, case, exact_fields, norm2,
                              transform_bound)
from test_isolated_potential import UNITS

pytestmark = pytest.mark.gpu
# the closed forms: a line of 64, 256, 512 and 1024, every pass as the long one, a 64 KiB launch
# and the cube
CLOSED = [ROLES[64]["y"], ROLES[256]["y"], ROLES[512]["z"], ROLES[1024]["y"], CUBE]
AMPLITUDE = 2.0 ** -3


def on_device(ctx, array):
    return torch.from_numpy(np.ascontiguousarray(array)).to(ctx.device)


def differing(got, want):
    """Where two float64 arrays differ by bits (a NaN equals a NaN of the same payload)."""
    return np.argwhere(np.ascontiguousarray(got).view(np.uint64) !=
                       np.ascontiguousarray(want).view(np.uint64))


def off_centre(shape):
    """An odd cell off the centre, (nz - 1, ny / 2 + 1, 3), clipped to the grid."""
    nz, ny, nx = shape
    return (nz - 1, min(ny // 2 + 1, ny - 1), min(3, nx - 1))


def test_the_shapes_are_the_ones_the_closed_forms_and_the_full_lds_cases_name():
    assert len(SHAPES) == 16 == len(set(SHAPES)) and set(CLOSED) <= set(SHAPES)
    assert FULL_LDS == [(2, 1024, 8), (1024, 2, 4)] and FULL_LDS[0] in CLOSED


# ---- by bits against the restatements --------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_fft3d_equals_the_restatement_by_bits(ctx, shape):
    """On FULL_LDS a strided pass asks for 65536 bytes of LDS: a refused launch raises here."""
    values, want, _ = case(shape)
    spectrum = ctx.fft3d(on_device(ctx, values))
    ctx.synchronize()
    got = spectrum.cpu().numpy()
    assert got.shape == shape + (2,) and got.dtype == np.float64
    different = differing(got, want)
    print(shape, "differing components:", len(different), different[:4].tolist())
    assert len(different) == 0


@pytest.mark.parametrize("shape", SHAPES)
def test_ifft3d_equals_the_restatement_by_bits(ctx, shape):
    _, spectrum, (want_real, want_imag) = case(shape)
    real, imag = ctx.ifft3d(on_device(ctx, spectrum), with_imag=True)
    alone = ctx.ifft3d(on_device(ctx, spectrum))
    ctx.synchronize()
    for got, want in ((real, want_real), (imag, want_imag), (alone, want_real)):
        different = differing(got.cpu().numpy(), want)
        print(shape, "differing cells:", len(different), different[:4].tolist())
        assert got.shape == shape and got.dtype == torch.float64 and len(different) == 0


# ---- closed forms, which do not go through the restatements ----------------------------------------

@pytest.mark.parametrize("shape", CLOSED)
def test_a_delta_off_the_centre_gives_its_closed_form(ctx, shape):
    """Every mode depends on the one cell through the whole address path: a misplaced element is
    an error of the size of the amplitude.  ||F - closed form|| <= 16 log2(Ntot) 2^-53 A sqrt
    Ntot, the transform's a-priori bound on the spectrum's norm."""
    at = off_centre(shape)
    values = np.zeros(shape)
    values[at] = AMPLITUDE
    spectrum = ctx.fft3d(on_device(ctx, values))
    ctx.synchronize()
    got = spectrum.cpu().numpy()
    want = fr.delta_spectrum(shape, at, AMPLITUDE)
    cells = values.size
    norm = AMPLITUDE * math.sqrt(cells)
    error = norm2(got[..., 0] - want[0], got[..., 1] - want[1])
    print(shape, at, "error / (2^-53 norm):", error / (EPS * norm), "bound:",
          transform_bound(cells, norm) / (EPS * norm))
    assert abs(norm2(*want) - norm) <= 2.0 ** -50 * norm
    assert error <= transform_bound(cells, norm)


@pytest.mark.parametrize("shape", CLOSED)
def test_one_mode_gives_its_plane_wave(ctx, shape):
    """The mirror: (A, 0) in one mode off the centre, zeros elsewhere; the inverse is (A / Ntot)
    exp(+2 pi i ...) with the norm A / sqrt Ntot."""
    at = off_centre(shape)
    spectrum = np.zeros(shape + (2,))
    spectrum[at + (0,)] = AMPLITUDE
    real, imag = ctx.ifft3d(on_device(ctx, spectrum), with_imag=True)
    alone = ctx.ifft3d(on_device(ctx, spectrum))
    ctx.synchronize()
    want = fr.plane_wave(shape, at, AMPLITUDE)
    cells = real.numel()
    norm = AMPLITUDE / math.sqrt(cells)
    error = norm2(real.cpu().numpy() - want[0], imag.cpu().numpy() - want[1])
    print(shape, at, "error / (2^-53 norm):", error / (EPS * norm), "bound:",
          transform_bound(cells, norm) / (EPS * norm))
    assert abs(norm2(*want) - norm) <= 2.0 ** -50 * norm
    assert error <= transform_bound(cells, norm)
    assert torch.equal(alone.view(torch.int64), real.view(torch.int64))


# ---- exact answers ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shape, axis", EXACT)
def test_fields_whose_transform_is_known_exactly(ctx, shape, axis):
    """Compared as values: a zero of either sign is a zero."""
    for name, (values, want) in exact_fields(shape, axis).items():
        spectrum = ctx.fft3d(on_device(ctx, values))
        ctx.synchronize()
        got = spectrum.cpu().numpy()
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:4].tolist())
        assert got[0, 0, 0, 1] == 0.0, name
    ones, delta = exact_fields(shape, axis)["a unit delta at the origin"][::-1]
    real, imag = ctx.ifft3d(on_device(ctx, ones), with_imag=True)
    ctx.synchronize()
    assert np.array_equal(real.cpu().numpy(), delta) and not imag.cpu().numpy().any()


# ---- there and back --------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES)
def test_a_round_trip_gives_the_field_back_within_the_a_priori_bound(ctx, shape):
    """||ifft3d(fft3d(x)) - x|| <= 32 log2(Ntot) 2^-53 ||x||: the forward bound plus the
    inverse's."""
    values = case(shape)[0]
    back, imag = ctx.ifft3d(ctx.fft3d(on_device(ctx, values)), with_imag=True)
    ctx.synchronize()
    norm = norm2(values)
    error, left = norm2(back.cpu().numpy() - values), norm2(imag.cpu().numpy())
    bound = 2.0 * transform_bound(values.size, norm)
    print(shape, "error, imag / (2^-53 norm):", error / (EPS * norm), left / (EPS * norm),
          "bound:", bound / (EPS * norm))
    assert error <= bound and left <= bound


# ---- one chain at a production length --------------------------------------------------------------

def test_a_point_mass_in_a_region_padded_to_a_line_of_128(ctx):
    """The calls api.isolated_potential_scene chains, on a 40 x 3 x 2 region (padded to 128 x 8 x
    4): the analytic scale / r of the offsets within the bound of
    test_isolated_potential.test_a_point_mass_gives_the_shifted_green_function, and the
    restatement by bits."""
    dims, size, at = (40, 3, 2), (0.5, 0.25, 1.0), (1, 2, 37)        # at: (k, j, i)
    nx, ny, nz = dims
    rho = np.zeros((nz, ny, nx))
    rho[at] = 3.0
    scale, self_value = ir.host_values(-2.0, size)
    want = ir.isolated_potential(rho, size, scale, self_value)
    padded = want["padded_dims"]
    assert padded == (128, 8, 4)
    grid = torch.zeros(padded[::-1], dtype=torch.float64, device=ctx.device)
    grid[:nz, :ny, :nx] = on_device(ctx, rho)
    spectrum = ctx.fft3d(grid)
    kernel = ctx.fft3d(ctx.isolated_green(padded, size, scale, self_value))
    ctx.spectrum_multiply(spectrum, kernel)
    real, imag = ctx.ifft3d(spectrum, with_imag=True)
    ctx.synchronize()
    got = real[:nz, :ny, :nx].contiguous().cpu().numpy()
    left = imag[:nz, :ny, :nx].contiguous().cpu().numpy()
    bound = UNITS * ir.unit(want)
    worst = 0.0
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                r = math.sqrt(((i - at[2]) * size[0]) ** 2 + ((j - at[1]) * size[1]) ** 2 +
                              ((k - at[0]) * size[2]) ** 2)
                analytic = 3.0 * scale / r if r else 0.0
                worst = max(worst, abs(got[k, j, i] - analytic))
    print("a point mass: distance", worst, "bound", bound, "imag_max", float(np.abs(left).max()))
    assert 0.0 < bound and worst <= bound and float(np.abs(left).max()) <= bound
    assert len(differing(got, want["potential"])) == 0
    assert len(differing(left, want["imag"])) == 0
