"""Structure functions on the GPU: structure_functions_kernel (csrc/avr_structure.hip) through
avr_grid_structure_functions, Context.structure_functions, api.structure_function_scene and
api.structure_functions, against the numpy restatement of the definition (structure_reference).
Counts are equal; a pair alone in its sum is equal to the reference's term by bits; every other
sum lies within the a-priori bound of adding n non-negative terms in any order around a math.fsum
of the reference's terms."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, plotfile, structure

import covering_grid_reference as cg
import derive_reference
import gradient_reference as ref
import structure_reference as sr

pytestmark = pytest.mark.gpu
VARIABLES = list(ref.VARIABLES)
SIZE = (0.5, 0.25, 1.0)          # (dx, dy, dz)
GROUP = 16384                    # csrc/avr_internal.h: kStructureGroupCells
# (nz, ny, nx): a row that is no multiple of a wave; rows of exactly a workgroup's stride; one
# long row; a column alone; a small power of two; more than two workgroups' shares with a partial
# third, rows of an odd length
SHAPES = [(3, 5, 131), (2, 2, 256), (1, 1, 1000), (5, 1, 1), (4, 8, 16), (40, 33, 29)]
assert 2 * GROUP < 40 * 33 * 29 < 3 * GROUP


@pytest.fixture(autouse=True)
def _empty_registries():
    def clear():
        for name in list(api.derived_fields()):
            api.remove_field(name)
    clear()
    yield
    clear()


def lags_of(shape):
    """Both signs along every axis that has two cells, |l_d| = N_d - 1 on every axis at once with
    one sign and with mixed signs, and a short diagonal of mixed signs."""
    n = shape[::-1]                                   # (nx, ny, nz)
    lags = []
    for d in range(3):
        if n[d] > 1:
            for step in (1, -min(3, n[d] - 1)):
                lag = [0, 0, 0]
                lag[d] = step
                lags.append(tuple(lag))
    far = tuple(v - 1 for v in n)
    short = tuple(min(2, v - 1) for v in n)
    for lag in (far, (-far[0], far[1], -far[2]), (far[0], -far[1], far[2]),
                (short[0], -short[1], short[2]), (-short[0], -short[1], short[2])):
        if lag not in lags and tuple(-v for v in lag) not in lags:
            lags.append(lag)
    return np.array(lags, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def grids_of(shape):
    """Three grids of a shape with values over six decades, made once; read-only."""
    rng = np.random.default_rng(sum(shape))
    return tuple(rng.standard_normal(shape) * 10.0 ** rng.uniform(-3.0, 3.0, shape)
                 for _ in range(3))


@functools.lru_cache(maxsize=None)
def case(shape, kinds, periodic, max_order=6):
    """(grids, lags, directions, the reference's results) of a shape, made once; read-only."""
    grids = grids_of(shape)[:kinds]
    lags = lags_of(shape)
    units = structure.unit_directions(lags, SIZE) if kinds == 3 else None
    return grids, lags, units, sr.structure_functions(grids, lags, units, max_order, periodic)


def on_device(ctx, array):
    return torch.from_numpy(np.ascontiguousarray(array)).to(ctx.device)


def run(ctx, grids, lags, units, max_order, periodic, out=None):
    found = ctx.structure_functions([on_device(ctx, g) for g in grids], lags, units, max_order,
                                    periodic, out)
    ctx.synchronize()
    return tuple(t.cpu().numpy() for t in found)


def check(got, want, before=None):
    """got = (pairs, sums, totals) as numpy arrays against the reference's results; before: what
    the outputs held."""
    pairs, sums, totals, terms = want
    had_pairs, had_sums, had_totals = before or (0, np.zeros_like(sums), 0)
    assert got[0].dtype == np.int64 and got[2].dtype == np.int64
    assert np.array_equal(got[0] - had_pairs, pairs)
    assert (got[2] - had_totals).tolist() == list(totals)
    assert got[1].shape == sums.shape
    worst = 0.0
    for m in range(sums.shape[0]):
        for kind in range(sums.shape[1]):
            for p in range(sums.shape[2]):
                total, had = float(sums[m, kind, p]), float(had_sums[m, kind, p])
                limit = sr.bound(int(pairs[m]), total, had)
                error = abs(got[1][m, kind, p] - had - total)
                if total:
                    worst = max(worst, error / (sr.U * total))
                assert error <= limit, (m, kind, p, got[1][m, kind, p], total, limit)
    print("worst error in units of 2^-53 of the sum:", worst, "pairs:", pairs.tolist()[:8])


# ---- 1. the kernel against the reference ---------------------------------------------------------

@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("kinds", [1, 3])
@pytest.mark.parametrize("shape", SHAPES)
def test_counts_are_equal_and_sums_within_the_bound(ctx, shape, kinds, periodic):
    grids, lags, units, want = case(shape, kinds, periodic)
    got = run(ctx, grids, lags, units, 6, periodic)
    check(got, want)
    cells = shape[0] * shape[1] * shape[2]
    assert int(got[0].sum()) + int(got[2].sum()) == len(lags) * cells
    if periodic:
        assert got[2].tolist() == [0, 0] and got[0].tolist() == [cells] * len(lags)
    else:
        assert got[2][0] > 0


@pytest.mark.parametrize("max_order", [1, 8])
def test_orders_one_and_eight(ctx, max_order):
    for kinds in (1, 3):
        grids, lags, units, want = case((3, 5, 131), kinds, True, max_order)
        got = run(ctx, grids, lags, units, max_order, True)
        assert got[1].shape == (len(lags), kinds, max_order) and np.isfinite(got[1]).all()
        check(got, want)


def test_one_lag_and_four_thousand_and_ninety_six(ctx):
    shape = (4, 8, 16)
    grids = grids_of(shape)
    for kinds, lags in ((3, [(-15, 7, -3)]), (1, [(1, 0, 0)])):
        units = structure.unit_directions(lags, SIZE) if kinds == 3 else None
        want = sr.structure_functions(grids[:kinds], lags, units, 6, False)
        check(run(ctx, grids[:kinds], lags, units, 6, False), want)
    every = [(x, y, z) for z in range(-3, 4) for y in range(-7, 8) for x in range(-15, 16)
             if (x, y, z) != (0, 0, 0)]
    lags = np.array((every + every)[:4096], dtype=np.int32)          # 3254 distinct lags
    assert lags.shape == (4096, 3)
    for periodic in (False, True):
        want = sr.structure_functions(grids[:1], lags, None, 2, periodic)
        check(run(ctx, grids[:1], lags, None, 2, periodic), want)
    units = structure.unit_directions(lags, SIZE)
    want = sr.structure_functions(grids, lags[-700:], units[-700:], 1, True)
    got = run(ctx, grids, lags, units, 1, True)
    assert got[2].tolist() == [0, 0] and got[0].tolist() == [512] * 4096
    check((got[0][-700:], got[1][-700:], got[2]), want)     # periodic: no lag adds to the totals


def test_a_pair_alone_in_its_sum_is_the_reference_term_by_bits(ctx):
    """A 2 x 2 x 2 open grid and the eight corner-to-corner lags: each has exactly one pair, added
    to zeroed outputs, so every kind and order must equal the reference's term by bits -- a fused
    multiply-add or a reordered sum anywhere in a term shows here."""
    rng = np.random.default_rng(8)
    lags = np.array([(x, y, z) for x in (1, -1) for y in (1, -1) for z in (1, -1)], dtype=np.int32)
    for size in (SIZE, (0.3, 0.7, 0.45)):
        units = structure.unit_directions(lags, size)
        for trial in range(4):
            grids = [rng.standard_normal((2, 2, 2)) * 10.0 ** rng.uniform(-2.0, 2.0, (2, 2, 2))
                     for _ in range(3)]
            for kinds in (1, 3):
                u = units if kinds == 3 else None
                pairs, sums, totals, terms = sr.structure_functions(grids[:kinds], lags, u, 8)
                assert pairs.tolist() == [1] * 8 and totals == (7 * 8, 0)
                got = run(ctx, grids[:kinds], lags, u, 8, False)
                assert got[0].tolist() == [1] * 8 and got[2].tolist() == [7 * 8, 0]
                for m in range(8):
                    assert ref.same_bits(got[1][m], terms[m][:, :, 0]), (size, trial, kinds, m)
                if kinds == 3:
                    assert (got[1][:, 1] > 0.0).any()       # a transverse part to be wrong about


@pytest.mark.parametrize("periodic", [False, True])
def test_an_integer_linear_field_by_bits(ctx, periodic):
    shape = (40, 33, 29)
    a, b, c = 3, -5, 7
    k, j, i = np.indices(shape)
    v = (a * i + b * j + c * k).astype(np.float64)
    lags = lags_of(shape)
    pairs, sums, totals = run(ctx, [v], lags, None, 4, periodic)
    if not periodic:      # every pair has the same increment: pairs |a lx + b ly + c lz|^p
        nz, ny, nx = shape
        for m, (lx, ly, lz) in enumerate(lags.tolist()):
            assert pairs[m] == (nx - abs(lx)) * (ny - abs(ly)) * (nz - abs(lz))
            step = abs(a * lx + b * ly + c * lz)
            for p in range(1, 5):
                assert pairs[m] * step ** p < 2 ** 53
                assert sums[m, 0, p - 1] == float(pairs[m] * step ** p), (m, p)
    # sums of integers below 2^53 are exact in any order: equal to the reference by bits
    want = sr.structure_functions([v], lags, None, 4, periodic)
    assert np.array_equal(pairs, want[0]) and totals.tolist() == list(want[2])
    assert float(want[1].max()) < 2.0 ** 53 and ref.same_bits(sums, want[1])


def test_prefilled_outputs_are_added_to(ctx):
    shape = (4, 8, 16)
    for kinds, periodic in ((1, False), (3, True)):
        grids, lags, units, want = case(shape, kinds, periodic)
        rng = np.random.default_rng(kinds)
        had = (rng.integers(0, 1000, len(lags)), rng.uniform(0.0, 1e3, want[1].shape),
               np.array([11, 7], dtype=np.int64))
        out = tuple(on_device(ctx, a) for a in had)
        got = run(ctx, grids, lags, units, 6, periodic, out)
        check(got, want, had)
        # the tensors handed in are the ones returned, and a second call adds again
        found = ctx.structure_functions([on_device(ctx, g) for g in grids], lags, units, 6,
                                        periodic, out)
        assert all(a is b for a, b in zip(found, out))
        ctx.synchronize()
        assert np.array_equal(out[0].cpu().numpy() - had[0], 2 * want[0])
        assert (out[2].cpu().numpy() - had[2]).tolist() == [2 * v for v in want[2]]


@pytest.mark.parametrize("periodic", [False, True])
def test_cells_that_are_not_finite_are_counted_exactly(ctx, periodic):
    shape = (3, 5, 131)
    grids = [g.copy() for g in grids_of(shape)]
    rng = np.random.default_rng(5)
    for g, value in zip(grids, (math.nan, math.inf, -math.inf)):
        g.reshape(-1)[rng.choice(g.size, 9, replace=False)] = value
    grids[0].reshape(-1)[:3] = (math.inf, math.inf, -math.inf)   # inf - inf and inf + inf
    grids[1][1, 2, 3] = 1e200                                   # finite, its square is not
    lags = lags_of(shape)
    units = structure.unit_directions(lags, SIZE)
    for kinds in (1, 3):
        u = units if kinds == 3 else None
        want = sr.structure_functions(grids[:kinds], lags, u, 6, periodic)
        assert want[2][1] > 0
        got = run(ctx, grids[:kinds], lags, u, 6, periodic)
        assert np.isfinite(got[1]).all()
        check(got, want)


def test_context_checks_its_arguments(ctx):
    grid = on_device(ctx, grids_of((4, 8, 16))[0])
    lags, units = [(1, 0, 0)], np.array([[1.0, 0.0, 0.0]])
    for wrong in (dict(components=[grid, grid]), dict(components=[grid.cpu()]),
                  dict(components=[grid.float()]), dict(components=[grid[:, :, ::2]]),
                  dict(components=[grid, grid, grid[:2]], directions=units),
                  dict(components=[grid.reshape(-1)]), dict(lags=[(1, 0)]), dict(lags=[]),
                  dict(lags=[(0.5, 0, 0)]), dict(directions=units),
                  dict(components=[grid, grid, grid]),
                  dict(components=[grid, grid, grid], directions=np.ones((2, 3))),
                  dict(max_order=0),
                  dict(out=(torch.zeros(2, dtype=torch.int64, device=ctx.device), None, None)),
                  dict(out=(None, torch.zeros((1, 1, 5), dtype=torch.float64, device=ctx.device),
                            None))):
        arguments = dict(components=[grid], lags=lags)
        arguments.update(wrong)
        with pytest.raises(ValueError):
            ctx.structure_functions(**arguments)
    for wrong, message in ((dict(lags=[(0, 0, 0)]), "a lag is zero"),
                           (dict(lags=[(16, 0, 0)]), "a lag spans a grid length"),
                           (dict(max_order=9), r"max_order must lie in \[1, 8\]"),
                           (dict(lags=np.ones((4097, 3), dtype=np.int32)), "n_lags must lie in")):
        arguments = dict(components=[grid], lags=lags)
        arguments.update(wrong)
        with pytest.raises(Exception, match=message):
            ctx.structure_functions(**arguments)
    # the components may alias each other
    got = ctx.structure_functions([grid, grid, grid], lags, units, 2)
    ctx.synchronize()
    assert got[0].tolist() == [15 * 8 * 4]


# ---- the C ABI -------------------------------------------------------------------------------------

def test_wrong_arguments_are_refused_and_the_outputs_untouched(ctx):
    grids, lags, units, want = case((4, 8, 16), 3, False)
    device = [on_device(ctx, g) for g in grids]
    n = len(lags)
    pairs = torch.full((n,), 7, dtype=torch.int64, device=ctx.device)
    sums = torch.full((n, 3, 6), 0.25, dtype=torch.float64, device=ctx.device)
    totals = torch.full((2,), 9, dtype=torch.int64, device=ctx.device)
    pointer = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    ints = lambda a: (None if a is None else
                      np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32)))
    doubles = lambda a: (None if a is None else
                         np.ascontiguousarray(a, np.float64).ctypes.data_as(C.POINTER(C.c_double)))

    def untouched():
        ctx.synchronize()
        return bool((pairs == 7).all()) and bool((sums == 0.25).all()) and \
            bool((totals == 9).all())

    def call(components=device, kinds=3, dims=(16, 8, 4), lags=lags, directions=units, n_lags=n,
             max_order=6, periodic=0, pairs=pairs, sums=sums, totals=totals):
        table = None
        if components is not None:
            table = (C.c_void_p * 3)(*[None if t is None else t.data_ptr() for t in components])
        return _capi.lib().avr_grid_structure_functions(
            ctx._handle, table, kinds, ints(dims), ints(lags), doubles(directions), n_lags,
            max_order, periodic, pointer(pairs), pointer(sums), pointer(totals))

    def spoilt(row, column, value, of=lags):
        changed = np.array(of, copy=True)
        changed[row, column] = value
        return changed

    flat = sums.view(-1)
    wrong = [
        (dict(components=None), "null argument"),
        (dict(components=[None, device[1], device[2]]), "null argument"),
        (dict(dims=None), "null argument"),
        (dict(lags=None), "null argument"),
        (dict(pairs=None), "null argument"),
        (dict(sums=None), "null argument"),
        (dict(totals=None), "null argument"),
        (dict(kinds=2), "n_components must be 1 or 3"),
        (dict(kinds=0), "n_components must be 1 or 3"),
        (dict(directions=None), "directions are given exactly when there are three components"),
        (dict(kinds=1), "directions are given exactly when there are three components"),
        (dict(components=[device[0], None, device[2]]), "null argument"),
        (dict(dims=(16, 0, 4)), "dims must be at least 1"),
        (dict(dims=(1 << 16, 1 << 15, 1)), "the grid has 2^31 cells or more"),
        (dict(n_lags=0), "n_lags must lie in [1, 4096]"),
        (dict(n_lags=4097), "n_lags must lie in [1, 4096]"),
        (dict(max_order=0), "max_order must lie in [1, 8]"),
        (dict(max_order=9), "max_order must lie in [1, 8]"),
        (dict(periodic=2), "periodic must be 0 or 1"),
        (dict(lags=spoilt(0, slice(None), 0)), "a lag is zero"),
        (dict(lags=spoilt(n - 1, 0, 16)), "a lag spans a grid length or more along an axis"),
        (dict(lags=spoilt(n - 1, 1, -8), periodic=1),
         "a lag spans a grid length or more along an axis"),
        (dict(lags=spoilt(1, 2, 4)), "a lag spans a grid length or more along an axis"),
        (dict(directions=spoilt(2, 1, math.nan, units)), "directions must be finite"),
        (dict(directions=spoilt(n - 1, 2, -math.inf, units)), "directions must be finite"),
        (dict(components=[device[0], device[1], flat]),
         "an output array overlaps a component grid"),
        (dict(pairs=device[1].view(torch.int64)), "an output array overlaps a component grid"),
        (dict(totals=device[2].view(torch.int64).view(-1)[510:]),
         "an output array overlaps a component grid"),
        (dict(totals=pairs[n - 1:]), "two output arrays overlap"),
        (dict(pairs=flat.view(torch.int64)[3:]), "two output arrays overlap"),
    ]
    for arguments, message in wrong:
        assert call(**arguments) == _capi.AVR_ERR_INVALID_ARGUMENT, arguments
        assert _capi.lib().avr_last_error().decode() == message, arguments
        assert untouched(), arguments
    # ... and the call that is in order adds to all three
    assert call() == 0
    ctx.synchronize()
    check((pairs.cpu().numpy(), sums.cpu().numpy(), totals.cpu().numpy()), want,
          (7, np.full(want[1].shape, 0.25), 9))


# ---- the API ---------------------------------------------------------------------------------------

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

    def check(self, got, names, level, lo, dims, lags=None, max_order=6, periodic=False,
              edges=None, min_level=0, fill=math.nan):
        """api.structure_functions' dict against the covering grids, then the per-lag results of
        the reference, then the bins of structure.bin_lags."""
        size = self.sizes[level]
        lags = structure.default_lags(dims) if lags is None else np.asarray(lags, dtype=np.int32)
        assert got["level"] == level and got["lo"] == lo and got["dims"] == dims
        assert got["cell_size"] == size and got["fields"] == tuple(names)
        assert got["max_order"] == max_order and got["periodic"] is periodic
        assert np.array_equal(got["lags"], lags) and got["lags"].dtype == np.int32
        assert ref.same_bits(got["r_lag"], structure.lag_lengths(lags, size))
        grids = [self.grid(name, level, lo, dims, min_level, fill) for name in names]
        assert got["absent"] == int((grids[0]["coverage"] == 0.0).sum())
        units = structure.unit_directions(lags, size) if len(names) == 3 else None
        want = sr.structure_functions([g["values"] for g in grids], lags, units, max_order,
                                      periodic)
        check((got["pairs_lag"], got["sums_lag"], np.array([got["outside"], got["nonfinite"]])),
              want)
        binned = structure.bin_lags(got["r_lag"], got["pairs_lag"], got["sums_lag"], edges)
        assert ref.same_bits(got["r"], binned["r"])
        assert np.array_equal(got["pairs"], binned["pairs"])
        assert ("r_edges" in got) == (edges is not None)
        if edges is not None:
            assert ref.same_bits(got["r_edges"], edges)
        assert list(got["S"]) == list(structure.kinds(len(names)))
        for kind, name in enumerate(got["S"]):
            assert got["S"][name].shape == (max_order, len(binned["r"]))
            assert ref.same_bits(got["S"][name], binned["S"][kind])
        return want


@pytest.fixture(scope="module")
def plot(tmp_path_factory):
    return Plot(tmp_path_factory.mktemp("structure") / "plt")


def test_api_structure_functions_of_stored_and_derived_fields_on_both_levels(ctx, plot, tmp_path):
    whole0, whole1 = ((0, 0, 0), (16, 8, 8)), ((0, 0, 0), (32, 16, 16))
    out = str(tmp_path / "structure.npz")
    got = api.structure_functions(plot.path, "u", level=0, output=out)
    plot.check(got, ["u"], 0, *whole0)
    assert len(got["lags"]) == 13 * 4 and list(got["S"]) == ["scalar"]
    assert got["outside"] > 0 and got["nonfinite"] == 0 and got["absent"] == 0
    # the second order is the mean of the squared increments: not below the squared first order
    assert (got["S"]["scalar"][1] >= got["S"]["scalar"][0] ** 2).all()

    back = structure.load_npz(out)
    assert set(back) == set(got) and list(back["S"]) == ["scalar"]
    for key in ("level", "lo", "dims", "cell_size", "fields", "max_order", "periodic", "outside",
                "nonfinite", "absent"):
        assert back[key] == got[key], key
    for key in ("lags", "pairs_lag", "pairs"):
        assert np.array_equal(back[key], got[key]), key
    for key in ("r_lag", "sums_lag", "r"):
        assert ref.same_bits(back[key], got[key]), key
    assert ref.same_bits(back["S"]["scalar"], got["S"]["scalar"])

    # the defaults: the finest loaded level, the whole domain; and periodic, where nothing is outside
    finest = api.structure_functions(plot.path, ["u"], periodic=True, max_order=3)
    plot.check(finest, ["u"], 1, *whole1, max_order=3, periodic=True)
    assert finest["outside"] == 0 and len(finest["lags"]) == 13 * 6
    coarse = api.structure_functions(plot.path, "u", max_level=0, max_order=1)
    assert coarse["level"] == 0 and coarse["dims"] == (16, 8, 8)

    # a derived field over a region that is no power of two, with lags and edges of the caller's
    api.add_field("uu", "u * u")
    region = ((3, 1, 2), (15, 7, 6))                   # 13 x 7 x 5 cells of level 1, across the patch
    lags = [(12, 0, 0), (-1, 6, -4), (0, 3, 0), (5, -2, 1), (0, 0, 2)]
    edges = np.array([0.0, 0.2, 0.5, 2.0])
    derived = api.structure_functions(plot.path, "uu", level=1, region=region, lags=lags,
                                      max_order=8, edges=edges)
    plot.check(derived, ["uu"], 1, region[0], (13, 7, 5), lags=lags, max_order=8, edges=edges)
    binned = api.structure_functions(plot.path, "uu", level=1, region=region, lags=lags,
                                     max_order=2, bins=3, r_range=(0.0, 1.5))
    plot.check(binned, ["uu"], 1, region[0], (13, 7, 5), lags=lags, max_order=2,
               edges=np.linspace(0.0, 1.5, 4))

    # a field with NaN and infinities: its pairs are left out and counted
    odd = api.structure_functions(plot.path, "odd", level=0, max_order=2)
    plot.check(odd, ["odd"], 0, *whole0, max_order=2)
    assert odd["nonfinite"] > 0 and np.isfinite(odd["sums_lag"]).all()


def test_api_structure_functions_of_three_components(ctx, plot):
    api.add_field("uu", "u * u")
    names = ["u", "whole", "uu"]
    size = plot.sizes[1]
    region = ((4, 2, 3), (14, 10, 9))                  # 11 x 9 x 7 cells of level 1
    left = tuple(LO[a] + region[0][a] * size[a] for a in range(3))
    right = tuple(LO[a] + (region[1][a] + 1) * size[a] for a in range(3))
    for periodic in (False, True):
        by_index = api.structure_functions(plot.path, names, level=1, region=region,
                                           periodic=periodic, max_order=4)
        by_edges = api.structure_functions(plot.path, names, level=1, left_edge=left,
                                           right_edge=right, periodic=periodic, max_order=4)
        for got in (by_index, by_edges):
            plot.check(got, names, 1, region[0], (11, 9, 7), max_order=4, periodic=periodic)
        assert list(by_index["S"]) == ["longitudinal", "transverse", "magnitude"]
        assert np.array_equal(by_index["sums_lag"] > 0, by_edges["sums_lag"] > 0)
    whole = api.structure_functions(plot.path, names, level=0, max_order=2)
    plot.check(whole, names, 0, (0, 0, 0), (16, 8, 8), max_order=2)
    # |dv|^2 = L^2 + T^2 up to rounding
    s = whole["S"]
    total = s["longitudinal"][1] + s["transverse"][1]
    assert np.allclose(total, s["magnitude"][1], rtol=1e-12, atol=0.0)


def test_cells_without_data_need_a_fill_value_and_nan_leaves_them_out(ctx, plot):
    whole1 = ((0, 0, 0), (32, 16, 16))
    with pytest.raises(ValueError, match="hold no data"):
        api.structure_functions(plot.path, "u", level=1, min_level=1)
    lags = [(1, 0, 0), (0, -2, 0), (3, 3, 3)]
    got = api.structure_functions(plot.path, "u", level=1, min_level=1, fill=math.nan, lags=lags,
                                  max_order=2)
    assert got["absent"] == 32 * 16 * 16 - 8 * 8 * 8
    want = plot.check(got, ["u"], 1, *whole1, lags=lags, max_order=2, min_level=1, fill=math.nan)
    # only the pairs inside the 8 x 8 x 8 patch count
    assert want[0].tolist() == [7 * 8 * 8, 8 * 6 * 8, 5 * 5 * 5] and got["nonfinite"] > 0
    zero = api.structure_functions(plot.path, "u", level=1, min_level=1, fill=0.0, lags=lags,
                                   max_order=2)
    plot.check(zero, ["u"], 1, *whole1, lags=lags, max_order=2, min_level=1, fill=0.0)
    assert zero["nonfinite"] == 0
