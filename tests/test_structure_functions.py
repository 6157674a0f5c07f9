"""Structure functions without a GPU: the numpy restatement of the definition
(structure_reference) against numbers known without it -- the pair counts of an open grid, an
integer linear field, a vector field along one axis, the periodic second order against an FFT
autocorrelation, a NaN cell; structure.py's lags, lengths, directions, bins and .npz file; the
refusals of api.structure_functions and api.structure_function_scene that come before any device
work; the declaration of the native entry."""
import math
import os

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, plotfile, structure
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds

import gradient_reference as ref
import structure_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
SHAPE = (5, 6, 7)                                   # (nz, ny, nx)
LAGS = [(1, 0, 0), (0, -1, 0), (0, 0, 1), (-6, 0, 0), (0, 5, 0), (0, 0, -4), (6, 5, 4),
        (2, -3, 1), (-1, 1, -1), (3, 0, -2)]


def field(shape, seed=3):
    rng = np.random.default_rng(sum(shape) + seed)
    return rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 3.0, shape)


# ---- the reference against numbers known without it ------------------------------------------------

def test_open_pair_counts_are_the_overlap_of_the_grid_with_itself_shifted():
    v = field(SHAPE)
    nz, ny, nx = SHAPE
    pairs, _, (outside, nonfinite), _ = sr.structure_functions([v], LAGS, max_order=2)
    want = [(nx - abs(lx)) * (ny - abs(ly)) * (nz - abs(lz)) for lx, ly, lz in LAGS]
    assert pairs.tolist() == want
    assert outside == len(LAGS) * v.size - sum(want) and nonfinite == 0
    pairs, _, totals, _ = sr.structure_functions([v], LAGS, max_order=2, periodic=True)
    assert pairs.tolist() == [v.size] * len(LAGS) and totals == (0, 0)


def test_an_integer_linear_field_gives_one_power_per_pair_exactly():
    a, b, c = 3, -5, 7
    k, j, i = np.indices(SHAPE)
    v = (a * i + b * j + c * k).astype(np.float64)
    pairs, sums, _, _ = sr.structure_functions([v], LAGS, max_order=8)
    for m, (lx, ly, lz) in enumerate(LAGS):
        step = abs(a * lx + b * ly + c * lz)
        for p in range(1, 9):
            assert pairs[m] * step ** p < 2 ** 53
            assert sums[m, 0, p - 1] == float(pairs[m] * step ** p), (m, p)


@pytest.mark.parametrize("periodic", [False, True])
def test_a_vector_field_along_the_lag_is_the_scalar_result_and_has_no_transverse_part(periodic):
    v, zero = field(SHAPE), np.zeros(SHAPE)
    for axis, lag in enumerate([(2, 0, 0), (0, -3, 0), (0, 0, 4)]):
        components = [zero, zero, zero]
        components[axis] = v
        u = np.zeros((1, 3))
        u[0, axis] = 1.0 if lag[axis] > 0 else -1.0
        pairs, sums, totals, _ = sr.structure_functions(components, [lag], u, 6, periodic)
        want = sr.structure_functions([v], [lag], None, 6, periodic)
        assert np.array_equal(pairs, want[0]) and totals == want[2]
        assert ref.same_bits(sums[:, 0], want[1][:, 0])         # longitudinal
        assert ref.same_bits(sums[:, 2], want[1][:, 0])         # magnitude
        assert not sums[:, 1].any()                             # transverse


def test_the_periodic_second_order_is_twice_the_variance_less_the_autocorrelation():
    """sum |dv|^2 = 2 (sum v^2 - sum v(x) v(x + l)) per component, the second sum read off the
    inverse transform of |F|^2.  The tolerance is a-priori, not measured: an element of the
    autocorrelation carries the forward transform's error twice (|F|^2) and the inverse's once,
    each 16 log2(N) 2^-53 of sum v^2 (the per-transform figure of DESIGN.md 7, "Power
    spectrum"), and sum v^2 its own N roundings; both enter twice.  The reference's sum is a
    correctly rounded fsum of terms that each carry three roundings relative to themselves."""
    shape = (4, 6, 10)
    components = [field(shape, seed) for seed in (1, 2, 3)]
    lags = [(1, 0, 0), (0, 2, 0), (0, 0, -3), (9, 5, 3), (-4, 1, 2), (5, 0, 0)]
    units = structure.unit_directions(lags, (1.0, 1.0, 1.0))
    pairs, sums, _, _ = sr.structure_functions(components, lags, units, 2, True)
    n = components[0].size
    assert pairs.tolist() == [n] * len(lags)
    squares = sum(math.fsum((v * v).reshape(-1)) for v in components)
    for m, (lx, ly, lz) in enumerate(lags):
        shifted = 0.0
        for v in components:
            spectrum = np.fft.fftn(v)
            correlation = np.fft.ifftn(spectrum * np.conj(spectrum)).real
            # sum_x v(x) v(x + l) sits at the index -l of the inverse of |F|^2 -- or at +l: it is even
            shifted += correlation[lz % shape[0], ly % shape[1], lx % shape[2]]
        want = 2.0 * (squares - shifted)
        tolerance = 2.0 * (3 * 16 * math.log2(n) + n) * U * squares + 4 * U * want
        assert abs(sums[m, 2, 1] - want) <= tolerance, (m, sums[m, 2, 1], want, tolerance)


def test_one_nan_cell_spoils_two_pairs_of_every_periodic_lag():
    v = field(SHAPE)
    v[2, 3, 4] = math.nan
    lags = LAGS
    pairs, sums, (outside, nonfinite), _ = sr.structure_functions([v], lags, max_order=3,
                                                                  periodic=True)
    assert outside == 0 and nonfinite == 2 * len(lags)
    assert pairs.tolist() == [v.size - 2] * len(lags) and np.isfinite(sums).all()
    units = structure.unit_directions(lags, (0.5, 0.25, 1.0))
    pairs, sums, (outside, nonfinite), _ = sr.structure_functions(
        [v, field(SHAPE, 1), field(SHAPE, 2)], lags, units, 3, True)
    assert nonfinite == 2 * len(lags) and pairs.tolist() == [v.size - 2] * len(lags)
    assert np.isfinite(sums).all()


def test_an_overflowing_square_counts_as_not_finite():
    v = np.zeros((1, 1, 4))
    v[0, 0, 1] = 1e200                                   # finite, its square is not
    pairs, sums, (outside, nonfinite), _ = sr.structure_functions(
        [v, v, v], [(1, 0, 0)], np.array([[1.0, 0.0, 0.0]]), 2, False)
    assert (pairs.tolist(), outside, nonfinite) == ([1], 1, 2) and not sums.any()
    pairs, sums, (outside, nonfinite), _ = sr.structure_functions([v], [(1, 0, 0)], None, 1)
    assert (pairs.tolist(), outside, nonfinite) == ([3], 1, 0) and sums[0, 0, 0] == 2e200


# ---- structure.py ----------------------------------------------------------------------------------

def test_the_default_lags_are_thirteen_directions_times_the_ladder():
    assert structure.ladder(128) == [1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128]
    assert structure.ladder(5) == [1, 2, 3, 4] and structure.ladder(1) == [1]
    assert structure.ladder(0) == []
    lags = structure.default_lags((256, 256, 256))
    assert lags.shape == (182, 3) and lags.dtype == np.int32
    rows = {tuple(row) for row in lags.tolist()}
    assert len(rows) == 182 and not any(tuple(-v for v in row) in rows for row in rows)
    assert np.abs(lags).max() == 128
    directions = {tuple(np.sign(row).tolist()) for row in lags}
    assert len(directions) == 13
    structure.check_lags(lags, (256, 256, 256))
    # in the plane only, and no further than half the shortest axis that has two cells
    plane = structure.default_lags((1, 8, 64))
    assert plane.shape == (16, 3) and not plane[:, 0].any()
    assert {tuple(np.sign(row).tolist()) for row in plane} == {(0, 1, 0), (0, 0, 1), (0, 1, 1),
                                                              (0, 1, -1)}
    assert sorted(set(np.abs(plane).max(axis=1).tolist())) == [1, 2, 3, 4]
    line = structure.default_lags((1, 1, 13))
    assert line.tolist() == [[0, 0, 1], [0, 0, 2], [0, 0, 3], [0, 0, 4], [0, 0, 6]]
    assert structure.default_lags((1, 1, 1)).shape == (0, 3)
    assert structure.default_lags((3, 3, 3)).shape == (13, 3)


def test_lags_are_checked():
    dims = (6, 5, 7)
    assert structure.check_lags([(5, -4, 6)], dims).tolist() == [[5, -4, 6]]
    assert structure.check_lags(np.array([[1.0, 0.0, 0.0]]), dims).dtype == np.int32
    for wrong in ([], [(0, 0, 0)], [(1, 0, 0), (0, 0, 0)], [(6, 0, 0)], [(0, -5, 0)], [(0, 0, 7)],
                  [(1, 0)], (1, 0, 0), [(0.5, 0, 0)], [(2 ** 31, 0, 0)],
                  np.ones((4097, 3), dtype=np.int32)):
        with pytest.raises(ValueError):
            structure.check_lags(wrong, dims)
    structure.check_lags(np.ones((4096, 3), dtype=np.int32), dims)
    for wrong in ((6, 5), (6, 0, 7), (2048, 1024, 1024)):
        with pytest.raises(ValueError):
            structure.check_dims(wrong)
    assert structure.check_dims((2 ** 31 - 1, 1, 1)) == (2 ** 31 - 1, 1, 1)
    assert structure.check_dims((7, 3, 5)) == (7, 3, 5)
    for wrong in (0, 9, -1):
        with pytest.raises(ValueError):
            structure.check_order(wrong)
    assert structure.check_order(8) == 8 and structure.check_order(1) == 1


def test_lengths_and_directions_are_formed_in_the_stated_order():
    size = (0.3, 0.7, 0.45)
    lags = [(1, 0, 0), (3, -2, 5), (0, 0, -7), (-4, 4, 4)]
    r = structure.lag_lengths(lags, size)
    u = structure.unit_directions(lags, size)
    for m, (lx, ly, lz) in enumerate(lags):
        r2 = float(lx * lx) * (0.3 * 0.3) + float(ly * ly) * (0.7 * 0.7)
        r2 = r2 + float(lz * lz) * (0.45 * 0.45)
        assert r[m] == math.sqrt(r2)
        assert u[m].tolist() == [(lx * 0.3) / r[m], (ly * 0.7) / r[m], (lz * 0.45) / r[m]]
        assert abs(float(u[m] @ u[m]) - 1.0) <= 4 * U
    assert u.flags["C_CONTIGUOUS"] and u.dtype == np.float64
    for wrong in ((1.0, 1.0), (1.0, 0.0, 1.0), (1.0, math.inf, 1.0)):
        with pytest.raises(ValueError):
            structure.lag_lengths(lags, wrong)


def test_lags_are_binned_by_distinct_length_and_by_edges():
    size = (1.0, 1.0, 1.0)
    lags = np.array([(1, 0, 0), (0, 2, 0), (0, 1, 0), (0, 0, -1), (1, 1, 0), (2, 0, 0),
                     (0, 1, -1)])
    r = structure.lag_lengths(lags, size)
    pairs = np.array([10, 20, 30, 40, 0, 60, 0], dtype=np.int64)
    sums = np.arange(7 * 3 * 2, dtype=np.float64).reshape(7, 3, 2) + 0.5
    got = structure.bin_lags(r, pairs, sums)
    assert got["r"].tolist() == [1.0, math.sqrt(2.0), 2.0] and got["lags_outside"] == 0
    assert got["pairs"].tolist() == [80, 0, 80]
    assert ref.same_bits(got["sums"][0], (sums[0] + sums[2]) + sums[3])
    assert ref.same_bits(got["sums"][2], sums[1] + sums[5])
    assert got["S"].shape == (3, 2, 3)
    assert ref.same_bits(got["S"][:, :, 0], got["sums"][0] / 80.0)
    assert np.isnan(got["S"][:, :, 1]).all()                      # no pairs: no moment
    # edges: e[i] <= r < e[i + 1], the last bin closed at the top; what lies beyond is counted
    edges = [1.0, math.sqrt(2.0), 2.0]
    got = structure.bin_lags(r, pairs, sums, edges)
    assert got["pairs"].tolist() == [80, 80] and got["lags_outside"] == 0
    assert ref.same_bits(got["r"], [0.5 * (1.0 + math.sqrt(2.0)), 0.5 * (math.sqrt(2.0) + 2.0)])
    assert ref.same_bits(got["sums"][1], ((sums[1] + sums[4]) + sums[5]) + sums[6])
    got = structure.bin_lags(r, pairs, sums, [1.1, 1.9])
    assert got["pairs"].tolist() == [0] and got["lags_outside"] == 5
    with pytest.raises(ValueError):
        structure.bin_lags(r, pairs[:3], sums)
    for wrong in ([1.0], [1.0, 1.0], [-1.0, 1.0], [2.0, 1.0], [0.0, math.inf]):
        with pytest.raises(ValueError):
            structure.check_edges(wrong)
    # the edges made from bins and a range
    assert structure.make_edges(r) is None
    assert ref.same_bits(structure.make_edges(r, bins=4), np.linspace(1.0, 2.0, 5))
    assert ref.same_bits(structure.make_edges(r, r_range=(0.5, 3.0)), np.linspace(0.5, 3.0, 4))
    assert ref.same_bits(structure.make_edges(r, 3, (0.5, 4.0), True), np.geomspace(0.5, 4.0, 4))
    for wrong in (dict(r_log=True), dict(bins=0), dict(bins=2049), dict(r_range=(2.0, 1.0)),
                  dict(r_range=(0.0, 1.0), r_log=True), dict(r_range=(0.0, math.inf))):
        with pytest.raises(ValueError):
            structure.make_edges(r, **wrong)


def test_the_npz_file_gives_back_what_was_saved(tmp_path):
    lags = structure.default_lags((6, 5, 7))
    r = structure.lag_lengths(lags, (0.5, 0.25, 1.0))
    rng = np.random.default_rng(4)
    sums = rng.uniform(0.0, 1.0, (len(lags), 3, 4))
    pairs = rng.integers(1, 99, len(lags))
    binned = structure.bin_lags(r, pairs, sums)
    found = {"level": 1, "lo": (3, -4, 8), "dims": (6, 5, 7), "cell_size": (0.5, 0.25, 1.0),
             "fields": ("vx", "vy", "vz"), "max_order": 4, "periodic": True, "lags": lags,
             "r_lag": r, "pairs_lag": pairs, "sums_lag": sums, "r": binned["r"],
             "r_edges": np.array([0.0, 1.0, 5.0]), "pairs": binned["pairs"],
             "S": dict(zip(structure.VECTOR_KINDS, binned["S"])), "outside": 12, "nonfinite": 3,
             "absent": 0}
    path = str(tmp_path / "structure.npz")
    structure.save_npz(found, path)
    back = structure.load_npz(path)
    assert set(back) == set(found) and set(back["S"]) == set(structure.VECTOR_KINDS)
    for key in ("level", "lo", "dims", "cell_size", "fields", "max_order", "periodic", "outside",
                "nonfinite", "absent"):
        assert back[key] == found[key] and type(back[key]) is type(found[key]), key
    for key in ("lags", "pairs_lag", "pairs"):
        assert np.array_equal(back[key], found[key]) and back[key].dtype == found[key].dtype
    for key in ("r_lag", "sums_lag", "r", "r_edges"):
        assert ref.same_bits(back[key], found[key]), key
    for kind in structure.VECTOR_KINDS:
        assert ref.same_bits(back["S"][kind], found["S"][kind])


# ---- the API's refusals ----------------------------------------------------------------------------

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
             dict(max_order=0), dict(max_order=9),
             dict(lags=[(0, 0, 0)]), dict(lags=[(1, 0)]), dict(lags=[]),
             dict(region=region, lags=[(5, 0, 0)]), dict(region=region, lags=[(0, 0, -6)]),
             dict(lags=np.ones((4097, 3), dtype=np.int32)),
             dict(region=((0, 0, 0), (0, 0, 0))),                  # one cell: no lag at all
             dict(edges=[0.0, 1.0], bins=3), dict(edges=[0.0, 1.0], r_range=(0.0, 1.0)),
             dict(edges=[0.0, 1.0], r_log=True), dict(edges=[1.0]), dict(edges=[1.0, 1.0]),
             dict(edges=[-1.0, 1.0]), dict(r_log=True), dict(bins=0), dict(bins=2049),
             dict(r_range=(1.0, 1.0)), dict(r_range=(0.0, 1.0), r_log=True)]
    for arguments in wrong:
        with pytest.raises(ValueError):
            api.structure_functions(path, "u", **arguments)
    for fields in ([], ["u", "whole"], ["u", "whole", "u", "whole"]):
        with pytest.raises(ValueError, match="one field or three"):
            api.structure_functions(path, fields)
    with pytest.raises(ValueError, match="max_order"):
        api.structure_functions(str(tmp_path / "none"), "u", max_order=12)
    with pytest.raises(RuntimeError):
        api.structure_functions(str(tmp_path / "none"), "u")
    with pytest.raises(RuntimeError):
        api.structure_functions(path, "no such field")
    with pytest.raises(RuntimeError):
        api.structure_functions(path, ["u", "whole", "no such field"])
    # ... and what is in order reaches the loader: no power of two is asked for
    for arguments in (dict(), dict(level=0, region=region), dict(level=1, **corners),
                      dict(region=region, lags=[(4, -6, 5)], periodic=True),
                      dict(max_order=8, bins=5, r_log=True), dict(edges=[0.0, 0.5, 3.0]),
                      dict(region=((0, 0, 0), (0, 0, 4)), fill=math.nan)):
        with pytest.raises(AssertionError, match="the runtime was touched"):
            api.structure_functions(path, "u", **arguments)
    with pytest.raises(AssertionError, match="the runtime was touched"):
        api.structure_functions(path, ["u", "whole", "u"])


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
        api.structure_function_scene(NoDevice(), full, 0, *arguments, rank=0, n_ranks=2)
    with pytest.raises(NotImplementedError):
        api.structure_function_scene(NoDevice(), part, 0, *arguments)
    with pytest.raises(NotImplementedError):
        api.structure_function_scene(NoDevice(), [full, full, part], 0, *arguments)
    for level, lo, dims in ((0, (0, 0, 0), (4, 0, 4)), (0, (0, 0), (4, 4, 4)),
                            (0, (0, 0, 0), (4, 4)), (1, (0, 0, 0), (4, 4, 4)),
                            (-1, (0, 0, 0), (4, 4, 4)), (0, (0, 0, 0), (1, 1, 1))):
        with pytest.raises(ValueError):
            api.structure_function_scene(NoDevice(), full, level, lo, dims, *arguments[2:])
    for wrong in (dict(max_order=0), dict(max_order=9), dict(lags=[(3, 0, 0)]),
                  dict(lags=[(0, 0, 0)]), dict(edges=[2.0, 1.0])):
        with pytest.raises(ValueError):
            api.structure_function_scene(NoDevice(), full, 0, *arguments, **wrong)
    with pytest.raises(ValueError, match="one field or three"):
        api.structure_function_scene(NoDevice(), [full, full], 0, *arguments)


# ---- the library's host side -------------------------------------------------------------------------

def test_the_entry_is_declared_and_exported(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    name = "avr_grid_structure_functions"
    declared = header.split(f"int {name}(")[1].split(");")[0]
    assert len(_capi.SIGNATURES[name][1]) == declared.count(",") + 1 == 12
    assert getattr(avr_lib, name) is not None
    assert avr_lib.avr_abi_version() == 2
