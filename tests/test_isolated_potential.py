"""The isolated potential without a GPU: the padding rule; the numpy restatement of the definition
(isolated_reference) against direct summation with math.fsum within an a-priori bound, against
clump binding's pairwise self-energy, on a point mass and with a self term; the written-out loop
of the Green's grid; spectra's .npz file; the refusals of api.isolated_potential that come before
any device work; the declarations of the native entries."""
import math
import os

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, plotfile, spectra
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds

import binding_reference as br
import gradient_reference as ref
import isolated_reference as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
# the bound of the reference around direct summation, in units of 2^-53 log2(Ptot) ||rho_pad||_2
# ||G||_2: the per-transform figure 32 of DESIGN.md 7 (two transforms of the round trip, "Inverse
# transform, Helmholtz split, potential") taken three times, plus 4 for the product's roundings.
# A-priori, not measured and not rigorous.
UNITS = 100.0
# (nx, ny, nz), (dx, dy, dz)
REGIONS = [((1, 1, 1), (0.5, 0.25, 1.0)), ((9, 3, 1), (0.5, 0.25, 1.0)),
           ((6, 5, 7), (0.5, 0.25, 1.0)), ((8, 8, 8), (1.0, 1.0, 1.0)),
           ((9, 10, 12), (0.3, 0.7, 0.45))]


def density(dims, seed=0):
    nx, ny, nz = dims
    return np.random.default_rng(sum(dims) + seed).standard_normal((nz, ny, nx))


# ---- the padding rule ------------------------------------------------------------------------------

def test_padded_dims_is_the_smallest_power_of_two_from_2n_minus_1():
    for n, p in ((1, 1), (2, 4), (3, 8), (4, 8), (5, 16), (512, 1024)):
        assert spectra.padded_dims((n, 1, n)) == (p, 1, p) == ir.padded_dims((n, 1, n))
        assert spectra.padded_dims((1, n, 1)) == (1, p, 1)
    for n in range(1, 513):
        p = spectra.padded_dims((n, n, n))[0]
        assert p & (p - 1) == 0 and p >= 2 * n - 1 and (p == 1 or p // 2 < 2 * n - 1)
        assert (p,) * 3 == ir.padded_dims((n, n, n))
    for wrong, axis in (((513, 4, 4), "x"), ((4, 0, 4), "y"), ((4, 4, -2), "z"),
                        ((4, 4, 1024), "z")):
        with pytest.raises(ValueError, match=f"512 cells along every axis.* along {axis}"):
            spectra.padded_dims(wrong)
    with pytest.raises(ValueError, match="three values"):
        spectra.padded_dims((4, 4))
    assert spectra.check_isolated_dims((5.0, 7, 6)) == (5, 7, 6)


# ---- the Green's grid ------------------------------------------------------------------------------

def test_the_loop_and_the_vectorised_green_grids_are_equal_by_bits():
    for padded, size, scale, self_value in (((16, 4, 8), (0.5, 0.25, 1.0), -0.3, 0.0),
                                            ((4, 1, 1), (0.3, 0.7, 0.45), 2.5, -1.25),
                                            ((1, 1, 1), (1.0, 1.0, 1.0), 1.0, 7.0)):
        g = ir.green(padded, size, scale, self_value)
        assert g.shape == padded[::-1] and g.dtype == np.float64
        assert ref.same_bits(g, ir.green_loops(padded, size, scale, self_value))
        assert g[0, 0, 0] == self_value and np.isfinite(g).all()
    g = ir.green((16, 4, 8), (0.5, 0.25, 1.0), -0.3)
    # even about every axis, the far corner is the cell (P / 2, P / 2, P / 2)
    assert g[3, 1, 5] == g[5, 3, 11] and g[4, 2, 8] == -0.3 / math.sqrt(16.0 + 0.25 + 16.0)
    assert g[0, 0, 1] == -0.3 / 0.5 and g[0, 0, 15] == g[0, 0, 1]


def test_the_host_values_are_formed_in_the_stated_order():
    size = (0.3, 0.7, 0.45)
    scale, self_value = ir.host_values(4.0 * math.pi, size, 2.0)
    volume = (0.3 * 0.7) * 0.45
    assert scale == -((4.0 * math.pi * volume) / (4.0 * math.pi)) and self_value == scale * 2.0
    assert ir.host_values(1.0, size) == (-(volume / (4.0 * math.pi)), -0.0)
    assert math.copysign(1.0, ir.host_values(-1.0, size)[1]) == 1.0


# ---- the reference against direct summation ----------------------------------------------------------

@pytest.mark.parametrize("dims,size", REGIONS)
def test_the_reference_against_direct_summation(dims, size):
    rho = density(dims)
    scale, _ = ir.host_values(1.0, size)
    got = ir.isolated_potential(rho, size, scale)
    want = ir.direct_sum(rho, size, scale)
    unit = ir.unit(got)
    distance = float(np.abs(got["potential"] - want).max())
    print(dims, "padded", got["padded_dims"], "max |phi|", float(np.abs(want).max()), "unit", unit,
          "distance", distance, "=", distance / unit if unit else 0.0, "units; imag_max",
          got["imag_max"], "=", got["imag_max"] / unit if unit else 0.0, "units")
    assert got["potential"].shape == rho.shape == got["imag"].shape
    assert got["padded_dims"] == spectra.padded_dims(dims)
    if dims == (1, 1, 1):
        assert not got["potential"].any() and not want.any() and got["imag_max"] == 0.0
    else:
        assert want.any()
    assert distance <= UNITS * unit
    assert got["imag_max"] <= UNITS * unit and got["imag_max"] == np.abs(got["imag"]).max()


# ---- the link to clump binding -----------------------------------------------------------------------

@pytest.mark.parametrize("dims,size", [REGIONS[2], REGIONS[3]])
def test_half_the_mass_weighted_potential_is_the_pairwise_self_energy(dims, size):
    nx, ny, nz = dims
    rng = np.random.default_rng(nx)
    m = rng.uniform(0.0, 1.0, (nz, ny, nx))
    m[rng.uniform(size=m.shape) < 0.2] = 0.0                      # cells without mass
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    x, y, z = ((index.astype(np.float64) + 0.5) * h for index, h in zip((i, j, k), size))
    w = br.self_energy(x.ravel(), y.ravel(), z.ravel(), m.ravel())
    phi = ir.isolated_potential(m, size, 1.0, 0.0)["potential"]
    half = 0.5 * math.fsum((m * phi).ravel().tolist())
    print(dims, "W", w, "0.5 sum m phi", half, "relative distance", abs(half - w) / w)
    assert w > 0.0 and abs(half - w) <= 8.0 * U * w


# ---- a point mass and the self term ------------------------------------------------------------------

def test_a_point_mass_gives_the_shifted_green_function():
    size, at = (0.5, 0.25, 1.0), (2, 1, 3)                        # at: (k, j, i)
    rho = np.zeros((4, 4, 4))
    rho[at] = 3.0
    scale, _ = ir.host_values(-2.0, size)
    got = ir.isolated_potential(rho, size, scale)
    bound = UNITS * ir.unit(got)
    worst = 0.0
    for k in range(4):
        for j in range(4):
            for i in range(4):
                r = math.sqrt(((i - at[2]) * size[0]) ** 2 + ((j - at[1]) * size[1]) ** 2 +
                              ((k - at[0]) * size[2]) ** 2)
                want = 3.0 * scale / r if r else 0.0
                worst = max(worst, abs(got["potential"][k, j, i] - want))
    print("a point mass: distance", worst, "bound", bound)
    assert 0.0 < bound and worst <= bound and got["imag_max"] <= bound


def test_a_self_term_shifts_the_potential_by_self_value_times_rho():
    dims, size = REGIONS[2]
    rho = density(dims, 1)
    scale, self_value = ir.host_values(1.0, size, 2.38 / 0.5)
    assert self_value < 0.0
    without = ir.isolated_potential(rho, size, scale)
    with_term = ir.isolated_potential(rho, size, scale, self_value)
    bound = UNITS * ir.unit(with_term)
    distance = float(np.abs(with_term["potential"] - without["potential"] - self_value * rho).max())
    print("a self term: distance", distance, "bound", bound)
    assert distance <= bound
    assert float(np.abs(with_term["potential"] -
                        ir.direct_sum(rho, size, scale, self_value)).max()) <= bound


def test_one_nan_cell_makes_the_whole_potential_nan():
    rho = density((3, 2, 2))
    rho[1, 0, 2] = math.nan
    got = ir.isolated_potential(rho, (1.0, 1.0, 1.0), -1.0)
    assert np.isnan(got["potential"]).all() and math.isnan(got["imag_max"])


# ---- the file ----------------------------------------------------------------------------------------

def test_the_npz_file_gives_back_what_was_saved(tmp_path):
    grid = np.arange(210.0).reshape(7, 5, 6)
    phi = {"level": 1, "lo": (3, -4, 8), "dims": (6, 5, 7), "padded_dims": (16, 16, 16),
           "cell_size": (0.5, 0.25, 1.0), "constant": -2.5, "self_term": 4.76, "potential": grid,
           "imag_max": 1e-17, "absent": 3}
    path = str(tmp_path / "isolated.npz")
    spectra.save_isolated_potential_npz(phi, path)
    assert os.path.exists(path) and not os.path.exists(path + ".npz")
    back = spectra.load_isolated_potential_npz(path)
    assert set(back) == set(phi) and ref.same_bits(back["potential"], grid)
    for key in ("level", "lo", "dims", "padded_dims", "cell_size", "constant", "self_term",
                "imag_max", "absent"):
        assert back[key] == phi[key] and type(back[key]) is type(phi[key]), key


# ---- refusals before any device work -----------------------------------------------------------------

DOMAINS = [((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))]
BOXES = [[((0, 0, 0), (15, 7, 7))], [((8, 4, 4), (15, 11, 11))]]
LO, HI, RATIO = (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), [2]


def test_the_api_refuses_wrong_arguments_before_anything_is_loaded(tmp_path, monkeypatch):
    path = str(tmp_path / "plt")
    plotfile.write_plotfile(path, list(ref.VARIABLES), ref.make_levels(DOMAINS, BOXES, RATIO, 3),
                            LO, HI, RATIO)

    def untouched(*args, **kwargs):
        raise AssertionError("the runtime was touched")

    monkeypatch.setattr(api, "_runtime_scope", untouched)
    monkeypatch.setattr(api, "_ensure_runtime", untouched)
    monkeypatch.setattr(api, "_load_variable_scenes", untouched)
    region = ((1, 0, 2), (5, 6, 7))                                # 5 x 7 x 6 cells
    corners = dict(left_edge=(0.0, 0.0, 0.0), right_edge=(0.75, 0.5, 0.5))
    wrong = [dict(region=region, **corners), dict(left_edge=corners["left_edge"]),
             dict(right_edge=corners["right_edge"]), dict(region=((0, 0, 0), (3, -1, 3))),
             dict(region=((0, 0), (3, 3))), dict(level=-1), dict(level=2),
             dict(region=((0, 0, 0), (512, 3, 3))),                # 513 cells along x
             dict(constant=math.inf), dict(constant=math.nan), dict(self_term=-1.0),
             dict(self_term=math.inf), dict(self_term=math.nan)]
    for arguments in wrong:
        with pytest.raises(ValueError):
            api.isolated_potential(path, "u", **arguments)
    with pytest.raises(ValueError, match="between 1 and 512 cells along every axis, not 513 "
                                         "along y"):
        api.isolated_potential(path, "u", region=((0, 0, 0), (3, 512, 3)))
    with pytest.raises(ValueError, match="not 600 along z"):
        api.isolated_potential(path, "u", level=0, region=((0, 0, -300), (3, 3, 299)))
    with pytest.raises(ValueError, match="constant"):
        api.isolated_potential(str(tmp_path / "none"), "u", constant=math.nan)
    with pytest.raises(ValueError, match="self_term"):
        api.isolated_potential(str(tmp_path / "none"), "u", self_term=-0.5)
    with pytest.raises(RuntimeError):
        api.isolated_potential(str(tmp_path / "none"), "u")
    with pytest.raises(RuntimeError):
        api.isolated_potential(path, "no such field")
    # ... and what is in order reaches the loader: no power of two is asked for
    for arguments in (dict(), dict(level=0, region=region), dict(level=1, **corners),
                      dict(region=((0, 0, 0), (511, 0, 2))), dict(constant=-4.0, self_term=4.76),
                      dict(self_term=0.0)):
        with pytest.raises(AssertionError, match="the runtime was touched"):
            api.isolated_potential(path, "u", **arguments)


def test_boxes_on_other_ranks_and_wrong_arguments_are_refused_before_device_work():
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"the context was used ({name})")

    box = AmrBox((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), level=0, dims=(4, 4, 4))
    bounds = VolumeBounds((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    full = api.SceneGeometry([box, box], [box, box], ScalarTransform(), bounds)
    part = api.SceneGeometry([box, box], [box], ScalarTransform(), bounds)
    arguments = ((0, 0, 0), (3, 4, 2), [(0.25, 0.25, 0.25)], (0.0, 0.0, 0.0), [])
    with pytest.raises(NotImplementedError):
        api.isolated_potential_scene(NoDevice(), full, 0, *arguments, rank=0, n_ranks=2)
    with pytest.raises(NotImplementedError):
        api.isolated_potential_scene(NoDevice(), part, 0, *arguments)
    for level, lo, dims in ((0, (0, 0, 0), (4, 0, 4)), (0, (0, 0), (4, 4, 4)),
                            (0, (0, 0, 0), (4, 513, 4)), (0, (0, 0, 0), (4, 4)),
                            (1, (0, 0, 0), (4, 4, 4)), (-1, (0, 0, 0), (4, 4, 4))):
        with pytest.raises(ValueError):
            api.isolated_potential_scene(NoDevice(), full, level, lo, dims, *arguments[2:])
    with pytest.raises(ValueError, match="constant"):
        api.isolated_potential_scene(NoDevice(), full, 0, *arguments, constant=math.inf)
    with pytest.raises(ValueError, match="self_term"):
        api.isolated_potential_scene(NoDevice(), full, 0, *arguments, self_term=-1e-300)


# ---- the library's host side -------------------------------------------------------------------------

def test_the_entries_are_declared_and_exported(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    for name, count in (("avr_isolated_green", 6), ("avr_spectrum_multiply", 4)):
        declared = header.split(f"int {name}(")[1].split(");")[0]
        assert len(_capi.SIGNATURES[name][1]) == declared.count(",") + 1 == count, name
        assert getattr(avr_lib, name) is not None
    assert avr_lib.avr_abi_version() == 2
