"""Phase plots and profiles, what needs no GPU: the C ABI's new entry and the unchanged ABI version,
api.bin_edges, the argument checks of api.phase / api.profile (raised before a plotfile is opened),
the host formulas on hand-made integer arrays, and the tests' own numpy reference
(tests/phase_reference.py) against a brute-force loop and against conservation."""
import inspect
import math

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, runtime

import phase_reference as ref


def test_new_symbol_resolves_and_has_a_prototype():
    handle = _capi.lib()
    assert getattr(handle, "avr_scene_joint_histogram") is not None
    assert "avr_scene_joint_histogram" in _capi.SIGNATURES
    assert len(_capi.SIGNATURES["avr_scene_joint_histogram"][1]) == 12
    assert hasattr(runtime.Scene, "joint_histogram")
    for name in ("bin_edges", "phase", "profile", "phase_scene", "combine_joint_histograms",
                 "validate_phase_arguments", "validate_profile_arguments"):
        assert callable(getattr(api, name)), name


def test_abi_version_stays_two():
    assert _capi.lib().avr_abi_version() == 2


def test_defaults():
    defaults = {k: p.default for k, p in inspect.signature(api.phase).parameters.items()}
    assert defaults["z"] == "cell_volume" and defaults["bins"] == (128, 128)
    assert defaults["x_log"] is False and defaults["log_scale"] is False
    assert defaults["min_level"] == 0 and defaults["max_level"] == -1 and defaults["output"] is None
    defaults = {k: p.default for k, p in inspect.signature(api.profile).parameters.items()}
    assert defaults["weight"] == "cell_volume" and defaults["bins"] == 128


# ---- bin_edges -------------------------------------------------------------------------------------

@pytest.mark.parametrize("lo,hi,n", [(-300.0, 300.0, 7), (0.1, 0.7, 128), (-1e-3, 5e7, 1024),
                                     (3.0, 4.0, 1), (-1e300, 1e300, 3)])
def test_linear_edges_are_the_formula_bit_for_bit(lo, hi, n):
    e = api.bin_edges(lo, hi, n)
    assert e.dtype == np.float64 and e.shape == (n + 1,)
    want = np.array([np.float64(lo) + (np.float64(hi) - np.float64(lo)) * (np.float64(i) / np.float64(n))
                     for i in range(n + 1)])
    assert np.array_equal(e[:-1].view(np.uint64), want[:-1].view(np.uint64))
    assert e[0] == lo and e[n] == hi
    assert np.array_equal(e, ref.linear_edges(lo, hi, n))


@pytest.mark.parametrize("lo,hi,n", [(1e-30, 1e30, 1024), (1e-3, 1e3, 5), (0.3, 0.9, 128),
                                     (2.0, 3.0, 1)])
def test_log_edges(lo, hi, n):
    e = api.bin_edges(lo, hi, n, log=True)
    assert e.dtype == np.float64 and e.shape == (n + 1,)
    assert e[0] == lo and e[n] == hi
    assert (e[1:] > e[:-1]).all()
    assert np.array_equal(e, ref.log_edges(lo, hi, n))
    assert np.allclose(np.log10(e), np.linspace(math.log10(lo), math.log10(hi), n + 1),
                       rtol=0.0, atol=1e-12)


@pytest.mark.parametrize("lo,hi,n,log", [(1.0, 1.0 + 4e-16, 8, False), (1.0, 1.0 + 4e-16, 8, True),
                                         (1e300, np.nextafter(1e300, 2e300), 2, False)])
def test_a_range_too_narrow_for_its_bins_is_refused(lo, hi, n, log):
    with pytest.raises(ValueError, match="strictly increasing"):
        api.bin_edges(lo, hi, n, log)


@pytest.mark.parametrize("args,match", [
    ((0.0, 1.0, 0), "integer"), ((0.0, 1.0, 1025), "integer"), ((0.0, 1.0, 2.5), "integer"),
    ((1.0, 1.0, 4), "lo < hi"), ((2.0, 1.0, 4), "lo < hi"), ((0.0, float("inf"), 4), "finite"),
    ((float("nan"), 1.0, 4), "finite"), ((0.0, 1.0, 4, True), "positive"),
    ((-1.0, 1.0, 4, True), "positive"),
])
def test_bin_edges_checks_its_arguments(args, match):
    with pytest.raises(ValueError, match=match):
        api.bin_edges(*args)


# ---- argument checks ---------------------------------------------------------------------------------

PHASE_BAD = [
    (dict(z=""), "z must"),
    (dict(z=3), "z must"),
    (dict(z=None), "z must"),
    (dict(bins=(0, 8)), "x bins"),
    (dict(bins=(8, 1025)), "y bins"),
    (dict(bins=(8, 2.5)), "y bins"),
    (dict(bins=8), "bins must hold two"),
    (dict(bins=(8, 8, 8)), "bins must hold two"),
    (dict(x_range=(1.0, 1.0)), "x_range must satisfy lo < hi"),
    (dict(y_range=(2.0, 1.0)), "y_range must satisfy lo < hi"),
    (dict(x_range=(0.0, float("inf"))), "x_range must be finite"),
    (dict(y_range=(float("nan"), 1.0)), "y_range must be finite"),
    (dict(x_range=(1.0,)), "x_range must hold two"),
    (dict(x_range=(0.0, 1.0), x_log=True), "x_range must be positive"),
    (dict(y_range=(-1.0, 1.0), y_log=True), "y_range must be positive"),
    (dict(x_edges=[0.0, 1.0, 1.0, 2.0]), "x_edges must be strictly increasing"),
    (dict(y_edges=[0.0, 2.0, 1.0]), "y_edges must be strictly increasing"),
    (dict(x_edges=[0.0, float("nan"), 1.0]), "x_edges must be finite"),
    (dict(x_edges=[1.0]), "x_edges must hold"),
    (dict(y_edges=list(range(1027))), "y_edges must hold"),
    (dict(value_range=(2.0, 1.0)), "lo < hi"),
    (dict(value_range=(0.0, 1.0), log_scale=True), "positive"),
]

PROFILE_BAD = [
    (dict(weight="mass"), "weight must be one of"),
    (dict(weight=None), "weight must be one of"),
    (dict(bins=0), "x bins"),
    (dict(bins=1025), "x bins"),
    (dict(bins=(4, 4)), "x bins"),
    (dict(x_range=(1.0, 1.0)), "lo < hi"),
    (dict(x_range=(0.0, float("-inf"))), "finite"),
    (dict(x_range=(0.0, 1.0), x_log=True), "positive"),
    (dict(x_edges=[3.0, 2.0]), "strictly increasing"),
]


def _no_gpu(monkeypatch):
    def no_gpu(*args, **kw):
        raise AssertionError("GPU work started")
    monkeypatch.setattr(api, "_runtime_scope", no_gpu)


@pytest.mark.parametrize("kwargs,match", PHASE_BAD)
def test_phase_refuses_bad_arguments_before_the_plotfile_is_opened(tmp_path, kwargs, match,
                                                                   monkeypatch):
    _no_gpu(monkeypatch)
    with pytest.raises(ValueError, match=match):
        api.phase(str(tmp_path / "missing"), "density", "temperature", **kwargs)


@pytest.mark.parametrize("kwargs,match", PROFILE_BAD)
def test_profile_refuses_bad_arguments_before_the_plotfile_is_opened(tmp_path, kwargs, match,
                                                                     monkeypatch):
    _no_gpu(monkeypatch)
    with pytest.raises(ValueError, match=match):
        api.profile(str(tmp_path / "missing"), "density", "temperature", **kwargs)


def test_too_many_bins_in_all_are_refused():
    # 1024 x 1024 is the limit and passes; explicit edges count like bins
    x, y, rng = api.validate_phase_arguments(bins=(1024, 1024))
    assert (x, y, rng) == ((1024, None, None), (1024, None, None), None)
    x, y, _ = api.validate_phase_arguments(bins=(3, 4), x_edges=[0.0, 1.0, 5.0], y_range=(1, 2),
                                           y_log=True)
    assert x[0] == 2 and x[1] is None and x[2].tolist() == [0.0, 1.0, 5.0]
    assert y == (4, (1.0, 2.0), None)
    assert api.validate_profile_arguments("cells", 7, (0, 1)) == (7, (0.0, 1.0), None)


def test_a_missing_plotfile_or_variable_is_a_runtime_error(tmp_path, monkeypatch):
    _no_gpu(monkeypatch)
    with pytest.raises(RuntimeError, match="does not exist"):
        api.phase(str(tmp_path / "missing"), "density", "temperature")
    with pytest.raises(RuntimeError, match="does not exist"):
        api.profile(str(tmp_path / "missing"), "density", "temperature")
    path = ref.write(tmp_path / "tiny", ref.tiny_levels())
    with pytest.raises(RuntimeError, match="Variable 'pressure' not found in plotfile"):
        api.phase(path, "density", "temperature", z="pressure")
    with pytest.raises(RuntimeError, match="Variable 'pressure' not found in plotfile"):
        api.profile(path, "density", "pressure")


# ---- host formulas on hand-made arrays ------------------------------------------------------------------

CELLS = np.array([[[1, 0, 4], [2, 3, 0]],
                  [[0, 0, 8], [16, 1, 0]],
                  [[0, 0, 0], [64, 0, 0]]], np.int64)                # [L = 3, ny = 2, nx = 3]
SUMS = np.array([[[3.0, 0.0, -8.0], [1.0, 6.0, 0.0]],
                 [[0.0, 0.0, 4.0], [-32.0, 5.0, 0.0]],
                 [[0.0, 0.0, 0.0], [128.0, 0.0, 0.0]]])
VOL = [0.5, 0.0625, 0.0078125]                                        # powers of two: exact


def test_values_from_the_per_level_arrays():
    assert api.joint_histogram_values(CELLS, None, VOL, "cell_volume").tolist() == \
        [[0.5, 0.0, 2.5], [2.5, 1.5625, 0.0]]
    assert api.joint_histogram_values(CELLS, SUMS, VOL, "cells").tolist() == \
        [[1.0, 0.0, 12.0], [82.0, 4.0, 0.0]]
    assert api.joint_histogram_values(CELLS, SUMS, VOL, "energy").tolist() == \
        [[1.5, 0.0, -3.75], [-0.5, 3.3125, 0.0]]
    with pytest.raises(ValueError):
        api.joint_histogram_values(CELLS, None, VOL, "energy")
    # the order of the sum: level ascending from +0.0, in float64
    vol = [0.1, 0.7, 1e-9]
    want = ((0.0 + 0.1 * 2.0) + 0.7 * 16.0) + 1e-9 * 64.0
    assert api.joint_histogram_values(CELLS, None, vol)[1, 0] == want


def test_profile_mean_and_its_empty_bins():
    mean, weight = api.profile_mean(CELLS[:, 1, :], SUMS[:, 1, :], VOL, "cell_volume")
    assert weight.tolist() == [2.5, 1.5625, 0.0]
    assert mean[:2].tolist() == [-0.5 / 2.5, 3.3125 / 1.5625] and math.isnan(mean[2])
    mean, weight = api.profile_mean(CELLS[:, 1, :], SUMS[:, 1, :], VOL, "cells")
    assert weight.tolist() == [82.0, 4.0, 0.0]
    assert mean[:2].tolist() == [97.0 / 82.0, 11.0 / 4.0] and math.isnan(mean[2])
    with pytest.raises(ValueError):
        api.profile_mean(CELLS[:, 1, :], SUMS[:, 1, :], VOL, "mass")


def test_combine_joint_histograms_is_the_plain_sum():
    totals = [np.array([1, 2], np.int64), np.array([10, 20], np.int64), np.array([0, 5], np.int64)]
    parts = [(CELLS * k, SUMS * k, t) for k, t in zip((1, 2, 3), totals)]
    cells, sums, total = api.combine_joint_histograms(parts)
    assert np.array_equal(cells, CELLS * 6) and cells.dtype == np.int64
    assert np.array_equal(sums, SUMS * 6.0) and total.tolist() == [11, 27]
    assert CELLS[0, 0, 0] == 1 and totals[0].tolist() == [1, 2]       # inputs are not written
    cells, sums, total = api.combine_joint_histograms([(CELLS, None, totals[0])])
    assert sums is None and np.array_equal(cells, CELLS)
    tensors = [tuple(torch.from_numpy(a) for a in p) for p in parts[:2]]
    cells, sums, total = api.combine_joint_histograms(tensors)
    assert isinstance(cells, torch.Tensor) and np.array_equal(cells.numpy(), CELLS * 3)
    assert np.array_equal(sums.numpy(), SUMS * 3.0) and total.tolist() == [11, 22]
    with pytest.raises(ValueError):
        api.combine_joint_histograms([])
    with pytest.raises(ValueError):
        api.combine_joint_histograms([parts[0], (CELLS, None, totals[0])])
    with pytest.raises(ValueError):
        api.combine_joint_histograms([parts[0], (CELLS[:2], SUMS[:2], totals[0])])


# ---- the tests' reference ----------------------------------------------------------------------------

@pytest.mark.parametrize("x,y,s", [(0, 1, 2), (0, None, 3), (1, 0, None)])
def test_the_numpy_reference_equals_a_brute_force_loop(x, y, s):
    levels = ref.tiny_levels()
    edges = {0: ref.X_EDGES, 1: ref.Y_EDGES}
    want = ref.brute_force(levels, x, y, s, edges[x], None if y is None else edges[y])
    got = ref.reference(levels, x, y, s, edges[x], None if y is None else edges[y])
    assert np.array_equal(got["cells"], want["cells"])
    assert (got["outside"], got["nonfinite"], got["uncovered"]) == \
        (want["outside"], want["nonfinite"], want["uncovered"])
    assert want["uncovered"] == 4 * 3 * 2 - 2 + 4 * 2 * 2 and want["cells"].sum() > 10
    if s is not None:
        for level in range(2):
            assert {b: sorted(v) for b, v in got["terms"][level].items()} == \
                {b: sorted(v) for b, v in want["terms"][level].items()}


@pytest.mark.parametrize("make", [ref.three_levels, ref.many_boxes])
def test_the_numpy_reference_conserves_cells_and_volume(make):
    levels = make()
    for lev in levels:                        # finite data: conservation is exact
        for data in lev["data"]:
            data[~np.isfinite(data)] = 1.0
    x_edges = api.bin_edges(-1e4, 1e4, 64)
    y_edges = api.bin_edges(1e-9, 1e9, 32, log=True)
    got = ref.reference(levels, 0, 1, None, x_edges, y_edges)
    assert got["outside"] == 0 and got["nonfinite"] == 0
    assert got["cells"].sum() == got["uncovered"]
    values = api.joint_histogram_values(got["cells"], None, ref.volumes(levels), "cell_volume")
    domain = math.prod(ref.PROB_HI[a] - ref.PROB_LO[a] for a in range(3))
    # each of the (bins + levels) additions and the products round once: a few hundred ulps at most
    assert abs(values.sum() - domain) <= 4096 * 2.0 ** -53 * domain
    # and with a range that cuts the data, every cell is still accounted for
    got = ref.reference(make(), 0, 1, 2, ref.X_EDGES, ref.Y_EDGES)
    assert got["outside"] > 0 and got["nonfinite"] > 0
    assert got["cells"].sum() + got["outside"] + got["nonfinite"] == got["uncovered"]


def test_the_fixtures_put_cells_on_every_explicit_edge():
    levels = ref.three_levels()
    density = np.concatenate([d[0].reshape(-1) for lev in levels for d in lev["data"]])
    temperature = np.concatenate([d[1].reshape(-1) for lev in levels for d in lev["data"]])
    for e in ref.X_EDGES:
        assert (density == e).sum() >= 1, e
    for e in ref.Y_EDGES:
        assert (temperature == e).sum() >= 1, e
    for field in (density, temperature):
        assert np.isnan(field).any() and np.isposinf(field).any() and np.isneginf(field).any()
