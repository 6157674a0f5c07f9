"""Grid fields without a GPU: the numpy reference (grid_field_reference) against numbers that are
known without it -- a linear function reproduced exactly, the two round trips through
covering_grid_reference, the totals of a region that leaves the domain counted cell by cell, clamp
against wrap at the region's faces --, the refusals of api.grid_scene, of the registry and of the
resolution that come before any device work, name collisions across the four registries, and the
declarations of the native entry."""
import math
import os

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, gridfields, plotfile
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds

import covering_grid_reference as cg
import gradient_reference as ref
import grid_field_reference as gf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIABLES = list(ref.VARIABLES)

THREE_DOMAINS = [((0, 0, 0), (11, 5, 7)), ((0, 0, 0), (23, 11, 15)), ((0, 0, 0), (47, 23, 31))]
# two fine boxes that touch at i = 11 | 12; the finest grid lies inside the first
THREE_BOXES = [[((0, 0, 0), (6, 5, 7)), ((7, 0, 0), (11, 5, 7))],
               [((4, 2, 2), (11, 7, 9)), ((12, 2, 2), (17, 9, 9))],
               [((12, 6, 6), (21, 13, 15))]]
THREE_LO, THREE_HI, THREE_RATIO = (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 2]
NAN_PAYLOAD = float(np.array([0x7ff8000000001234], dtype=np.uint64).view(np.float64)[0])


@pytest.fixture(autouse=True)
def _empty_registries():
    def clear():
        for name in list(api.grid_fields()):
            api.remove_grid_field(name)
        for name in list(api.clump_fields()):
            api.remove_clump_field(name)
        for name in list(api.gradient_fields()):
            api.remove_gradient_field(name)
        for name in list(api.derived_fields()):
            api.remove_field(name)
    clear()
    yield
    clear()


@pytest.fixture(scope="module")
def three():
    return ref.make_levels(THREE_DOMAINS, THREE_BOXES, THREE_RATIO, 71)


def leaves(levels, variable="u", **load):
    return ref.leaf_arrays(levels, THREE_RATIO, VARIABLES.index(variable), **load)[0]


# ---- the reference ---------------------------------------------------------------------------------

@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("periodic", [False, True])
def test_linear_interpolation_reproduces_a_linear_function_inside_the_region(three, level,
                                                                             periodic):
    """g = a + bx i + by j + bz k with small integers: every fine cell centre whose stencil lies
    inside the region gets the function's value there, exactly -- the centre of the level-l cell
    I lies at the level-L coordinate (I + 0.5) / R - 0.5, a multiple of 1 / (2 R)."""
    arrays = leaves(three)
    lo, dims = cg.whole_domain(three, THREE_RATIO, level)
    k, j, i = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in dims[::-1]), indexing="ij")
    a, b = 3.0, (2.0, -5.0, 7.0)
    grid = a + b[0] * i + b[1] * j + b[2] * k
    dense, outside, partial = gf.grid_scene_of(arrays, THREE_RATIO, grid, level, lo, 1, periodic)
    assert outside == 0 and partial == 0
    checked = 0
    for l in range(level + 1, 3):
        origin, mask, _ = arrays[l]
        refine = 2 ** (l - level)
        kk, jj, ii = np.nonzero(mask)
        at = [(np.stack([ii, jj, kk])[d] + origin[d] + 0.5) / refine - 0.5 for d in range(3)]
        interior = np.ones(kk.size, dtype=bool)
        for d in range(3):                   # both stencil cells inside [0, dims)
            interior &= (at[d] >= 0.0) & (at[d] <= dims[d] - 1.0)
        want = a + b[0] * at[0] + b[1] * at[1] + b[2] * at[2]
        got = dense[l][kk, jj, ii]
        assert np.array_equal(got[interior], want[interior])
        checked += int(interior.sum())
        if not interior.all():               # past the faces clamp and wrap are other functions
            assert not np.array_equal(got[~interior], want[~interior])
    assert checked >= 800


@pytest.mark.parametrize("variable", ["u", "whole"])
def test_a_covering_grid_at_the_finest_level_written_back_gives_every_leaf_by_bits(three,
                                                                                   variable):
    """A leaf of the finest level is copied.  A coarser leaf v comes back as the mean of R^3
    copies of v, added one by one: exact where every partial sum n v is a double (the integers of
    `whole`), and otherwise within (R^3 - 1) roundings of 2^-53 each, relative to v."""
    arrays = leaves(three, variable)
    lo, dims = cg.whole_domain(three, THREE_RATIO, 2)
    grid = cg.covering_grid_of(arrays, THREE_RATIO, 2, lo, dims)["values"]
    dense, outside, partial = gf.grid_scene_of(arrays, THREE_RATIO, grid, 2, lo)
    assert outside == 0 and partial == 0
    for level, ((_, mask, values), got) in enumerate(zip(arrays, dense)):
        assert mask.any()
        if level == 2 or variable == "whole":
            assert ref.same_bits(got[mask], values[mask])
        else:
            roundings = (2 ** (2 - level)) ** 3 - 1
            assert (np.abs(got[mask] - values[mask]) <=
                    roundings * 2.0 ** -53 * np.abs(values[mask])).all()


@pytest.mark.parametrize("level", [0, 1, 2])
@pytest.mark.parametrize("interpolation", [0, 1])
def test_a_grid_written_to_the_leaves_and_covered_again_is_the_grid_where_leaves_are_as_fine(
        three, level, interpolation):
    arrays = leaves(three)
    lo, dims = cg.whole_domain(three, THREE_RATIO, level)
    rng = np.random.default_rng(5)
    grid = rng.integers(-1000, 1001, size=dims[::-1]).astype(np.float64)
    dense, _, _ = gf.grid_scene_of(arrays, THREE_RATIO, grid, level, lo, interpolation)
    written = [(origin, mask, values) for (origin, mask, _), values in zip(arrays, dense)]
    back = cg.covering_grid_of(written, THREE_RATIO, level, lo, dims)
    fine = back["level"] >= level
    assert fine.any() and (level == 0) == bool(fine.all())
    if interpolation == 0:
        assert ref.same_bits(back["values"][fine], grid[fine])
    else:           # only the cells of the grid's own level are copied; finer ones are interpolated
        same = back["level"] == level
        assert same.any() and ref.same_bits(back["values"][same], grid[same])


def test_the_totals_of_a_region_that_leaves_the_domain_on_every_side(three):
    arrays = leaves(three)
    lo, dims = (-3, 3, 4), (29, 7, 5)            # level 1: i = -3 .. 25 of 0 .. 23
    grid = np.arange(29 * 7 * 5, dtype=np.float64).reshape(5, 7, 29)
    for interpolation in (0, 1):
        dense, outside, partial = gf.grid_scene_of(arrays, THREE_RATIO, grid, 1, lo, interpolation,
                                                   fill=-0.0)
        want_outside = want_partial = 0
        for l, (origin, mask, _) in enumerate(arrays):
            for k, j, i in zip(*np.nonzero(mask)):
                index = (i + origin[0], j + origin[1], k + origin[2])
                if l == 0:                        # the 8 children, one by one
                    n = sum(all(lo[d] <= 2 * index[d] + c[d] < lo[d] + dims[d] for d in range(3))
                            for c in np.ndindex(2, 2, 2))
                    want_outside += n == 0
                    want_partial += 0 < n < 8
                    filled = n == 0
                else:
                    g = [index[d] // 2 ** (l - 1) for d in range(3)]
                    filled = not all(lo[d] <= g[d] < lo[d] + dims[d] for d in range(3))
                    want_outside += filled
                got = dense[l][k, j, i]
                assert filled == (got == 0.0 and bool(np.signbit(got)))    # -0.0, by bits
        assert (outside, partial) == (want_outside, want_partial)
        assert outside > 500 and partial > 10


def test_clamped_and_wrapped_neighbours_at_the_faces_of_the_region():
    """One axis at a time: a 4 x 1 x 1 grid of level 0 under level-1 cells at ratio 2.  The cell
    I = 0 lies a quarter cell below the centre of grid cell 0: clamped it is g[0], wrapped it is
    g[0] + 0.25 * (g[3] - g[0])."""
    grid = np.array([[[8.0, 16.0, 32.0, 64.0]]])
    index = np.array([[0, 1, 2, 7, -1, 8], [0] * 6, [0] * 6])
    clamped, filled, _ = gf.grid_cells(grid, 0, (0, 0, 0), 1, index, [2], 1, False, -1.0)
    wrapped, _, _ = gf.grid_cells(grid, 0, (0, 0, 0), 1, index, [2], 1, True, -1.0)
    assert filled.tolist() == [False] * 4 + [True] * 2
    assert clamped.tolist() == [8.0, 10.0, 14.0, 64.0, -1.0, -1.0]
    assert wrapped.tolist() == [8.0 + 0.25 * 56.0, 10.0, 14.0, 64.0 + 0.25 * (8.0 - 64.0), -1.0, -1.0]
    # along y and z the same numbers
    for axis in (1, 2):
        turned = np.moveaxis(grid, 2, 2 - axis)
        moved = np.roll(index, axis, axis=0)
        again, _, _ = gf.grid_cells(turned, 0, (0, 0, 0), 1, moved, [2], 1, True, -1.0)
        assert again.tolist() == wrapped.tolist()
    # one cell wide: the wrapped neighbour is the cell itself
    alone, _, _ = gf.grid_cells(grid[:, :, :1], 0, (0, 0, 0), 1, index[:, :2], [2], 1, True)
    assert alone.tolist() == [8.0, 8.0]
    # an infinity next to the cell: a + t * (b - a) is carried out as it stands
    odd = np.array([[[1.0, np.inf, np.nan, -np.inf]]])
    got, _, _ = gf.grid_cells(odd, 0, (0, 0, 0), 1, index[:, :4], [2], 1, False)
    # 1 + 0.25 * (inf - 1) = inf along x, then inf + 0.25 * (inf - inf) along y: NaN
    assert got[0] == 1.0 and np.isnan(got[1:]).all()
    constant, _, _ = gf.grid_cells(odd, 0, (0, 0, 0), 1, index[:, :4], [2], 0, False)
    assert ref.same_bits(constant, np.array([1.0, 1.0, np.inf, -np.inf]))


def test_the_fill_value_keeps_its_bits_and_a_coarser_leaf_takes_the_mean_in_order():
    grid = np.array([[[1e16, 1.0], [-1e16, 1.0]], [[1.0, 1.0], [1.0, 1.0]]])
    index = np.array([[0, 1], [0, 0], [0, 0]])
    values, filled, partial = gf.grid_cells(grid, 1, (0, 0, 0), 0, index, [2], 0, False, NAN_PAYLOAD)
    # ((((((1e16 + 1) - 1e16) + 1) + 1) + 1) + 1) + 1 in k, j, i order: 1e16 + 1 rounds to 1e16
    assert values[0] == 5.0 / 8.0 and filled.tolist() == [False, True] and not partial.any()
    assert values.view(np.uint64)[1] == 0x7ff8000000001234
    part, _, partial = gf.grid_cells(grid, 1, (1, 0, 0), 0, index, [2], 0, False)
    # 4 of 8 children each: (1e16 - 1e16 + 1 + 1) / 4 at i = 1, four ones at i = 2
    assert part.tolist() == [0.5, 1.0] and partial.tolist() == [True, True]


# ---- refusals before any device work -----------------------------------------------------------

class NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the context was used ({name})")


def test_grid_scene_refuses_other_ranks_and_wrong_arguments_before_device_work():
    box = AmrBox((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), level=0, dims=(4, 4, 4))
    bounds = VolumeBounds((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    full = api.SceneGeometry([box, box], [box, box], ScalarTransform(), bounds)
    part = api.SceneGeometry([box, box], [box], ScalarTransform(), bounds)
    grid = np.zeros((4, 4, 4))
    levels = ([(0.25, 0.25, 0.25)], (0.0, 0.0, 0.0), [])
    with pytest.raises(NotImplementedError):
        api.grid_scene(NoDevice(), full, grid, 0, (0, 0, 0), *levels, rank=0, n_ranks=2)
    with pytest.raises(NotImplementedError):
        api.grid_scene(NoDevice(), part, grid, 0, (0, 0, 0), *levels)
    wrong = [dict(grid=np.zeros((4, 4))), dict(grid=np.zeros((4, 0, 4))), dict(lo=(0, 0)),
             dict(level=1), dict(level=-1), dict(interpolation="cubic"), dict(interpolation=1)]
    for changed in wrong:
        a = {**dict(grid=grid, level=0, lo=(0, 0, 0), interpolation="constant"), **changed}
        with pytest.raises(ValueError):
            api.grid_scene(NoDevice(), full, a["grid"], a["level"], a["lo"], *levels,
                           interpolation=a["interpolation"])


def test_the_registry_checks_its_arguments_when_registering():
    grid = np.zeros((2, 3, 4))
    wrong = [
        lambda: api.add_potential_field("", "u"),
        lambda: api.add_potential_field(3, "u"),
        lambda: api.add_potential_field("phi", ""),
        lambda: api.add_potential_field("phi", "u", constant=math.inf),
        lambda: api.add_potential_field("phi", "u", boundary="open"),
        lambda: api.add_potential_field("phi", "u", self_term=-1.0, boundary="isolated"),
        lambda: api.add_potential_field("phi", "u", self_term=1.0),            # periodic has none
        lambda: api.add_potential_field("phi", "u", level=-1),
        lambda: api.add_potential_field("phi", "u", level=0.5),
        lambda: api.add_potential_field("phi", "u", region=((0, 0, 0), (3, -1, 3))),
        lambda: api.add_potential_field("phi", "u", region=((0, 0), (3, 3))),
        lambda: api.add_potential_field("phi", "u", region=((0, 0, 0), (3, 3, 3)),
                                        left_edge=(0, 0, 0), right_edge=(1, 1, 1)),
        lambda: api.add_potential_field("phi", "u", left_edge=(0, 0, 0)),
        lambda: api.add_potential_field("phi", "u", left_edge=(0, 0, 0), right_edge=(1, math.nan, 1)),
        lambda: api.add_potential_field("phi", "u", interpolation="cubic"),
        lambda: api.add_helmholtz_field("s", ("u", "v")),
        lambda: api.add_helmholtz_field("s", ("u", "v", "")),
        lambda: api.add_helmholtz_field("s", ("u", "v", "w"), part="total"),
        lambda: api.add_helmholtz_field("s", ("u", "v", "w"), component="r"),
        lambda: api.add_helmholtz_field("s", ("u", "v", "w"), interpolation=1),
        lambda: api.add_array_field("g", grid, -1),
        lambda: api.add_array_field("g", grid, 16),
        lambda: api.add_array_field("g", grid, 0, lo=(0, 0)),
        lambda: api.add_array_field("g", grid[0], 0),
        lambda: api.add_array_field("g", grid[:, :0], 0),
        lambda: api.add_array_field("g", grid.astype(np.float32), 0),
        lambda: api.add_array_field("g", grid, 0, interpolation="nearest"),
    ]
    for call in wrong:
        with pytest.raises(ValueError):
            call()
    assert api.grid_fields() == {}
    api.add_potential_field("phi", "u", 2.0, "isolated", 1, ((0, 0, 0), (3, 3, 3)), self_term=0.5)
    api.add_helmholtz_field("s", ("u", "v", "w"), "compressive", "z")
    api.add_array_field("g", grid, 1, (-2, 0, 3), "linear", True, -1.0)
    found = api.grid_fields()
    assert list(found) == ["phi", "s", "g"] and gridfields.inputs_of("g") == ()
    assert found["phi"]["kind"] == "potential" and found["phi"]["periodic"] is False
    assert found["phi"]["interpolation"] == "linear" and found["phi"]["level"] == 1
    assert found["s"]["component"] == 2 and found["s"]["periodic"] is True
    assert gridfields.inputs_of("s") == ("u", "v", "w") and gridfields.inputs_of("phi") == ("u",)
    assert found["g"]["array"] is grid and found["g"]["lo"] == (-2, 0, 3)
    api.remove_grid_field("s")
    assert list(api.grid_fields()) == ["phi", "g"]
    with pytest.raises(KeyError):
        api.remove_grid_field("s")


def test_a_name_belongs_to_one_of_the_four_registries_and_cycles_are_refused():
    grid = np.zeros((2, 2, 2))
    adders = {"derived": lambda n: api.add_field(n, "u * 2"),
              "gradient": lambda n: api.add_gradient_field(n, "u", "x"),
              "clump": lambda n: api.add_clump_field(n, "u", 0.0),
              "potential": lambda n: api.add_potential_field(n, "u"),
              "helmholtz": lambda n: api.add_helmholtz_field(n, ("u", "v", "w")),
              "array": lambda n: api.add_array_field(n, grid, 0)}
    grid_kinds = ("potential", "helmholtz", "array")
    for first, add in adders.items():
        add("taken")
        for second, again in adders.items():
            if first in grid_kinds and second in grid_kinds:
                continue                    # a grid field may be registered anew, as a derived one
            if first == second:
                continue
            with pytest.raises(ValueError, match="is a registered"):
                again("taken")
        for remove in (api.remove_field, api.remove_gradient_field, api.remove_clump_field,
                       api.remove_grid_field):
            try:
                remove("taken")
            except KeyError:
                pass
    for name in ("x", "cell_volume", "sqrt", "cells", "field"):
        for kind in grid_kinds:
            with pytest.raises(ValueError, match="cannot name a grid field"):
                adders[kind](name)
    # a cycle through the registries, closed from either side
    api.add_field("rho2", "u + phi")
    with pytest.raises(ValueError, match="cycle"):
        api.add_potential_field("phi", "rho2")
    assert "phi" not in api.grid_fields()
    api.add_potential_field("psi", "rho3")
    with pytest.raises(ValueError, match="cycle"):
        api.add_field("rho3", "psi * 2")
    api.add_gradient_field("dpsi", "psi", "x")
    with pytest.raises(ValueError, match="cycle"):
        api.add_helmholtz_field("rho3", ("dpsi", "u", "u"))
    assert "rho3" not in api.grid_fields() and "rho3" not in api.derived_fields()


def test_a_plotfile_level_call_checks_a_grid_fields_inputs_before_anything_is_loaded(tmp_path,
                                                                                     monkeypatch,
                                                                                     three):
    path = str(tmp_path / "plt")
    plotfile.write_plotfile(path, VARIABLES, three, THREE_LO, THREE_HI, THREE_RATIO)

    def untouched(*args, **kwargs):
        raise AssertionError("the runtime was touched")

    monkeypatch.setattr(api, "_runtime_scope", untouched)
    monkeypatch.setattr(api, "_ensure_runtime", untouched)
    monkeypatch.setattr(api, "_load_variable_scenes", untouched)
    api.add_potential_field("phi", "no such density")
    api.add_helmholtz_field("s", ("u", "odd", "missing"))
    api.add_field("e", "0.5 * u * phi")
    for name, needed_by in (("phi", "grid field 'phi'"), ("s", "grid field 's'"),
                            ("e", "grid field 'phi'")):
        with pytest.raises(RuntimeError, match="not found in plotfile") as refused:
            api.covering_grid(path, 0, [name])
        assert needed_by in str(refused.value)
    # ... and what is in order reaches the loader
    api.add_potential_field("phi", "u")
    api.add_array_field("g", np.zeros((2, 2, 2)), 0)
    for name in ("phi", "e", "g"):
        with pytest.raises(AssertionError, match="the runtime was touched"):
            api.covering_grid(path, 0, [name])


# ---- declarations ------------------------------------------------------------------------------------

def test_the_entry_is_declared_and_exported(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    assert "int avr_scene_grid_field(avr_context *ctx, avr_scene *out, const double *grid_dev" in header
    declared = header.split("int avr_scene_grid_field(")[1].split(");")[0]
    assert len(_capi.SIGNATURES["avr_scene_grid_field"][1]) == declared.count(",") + 1 == 13
    assert getattr(avr_lib, "avr_scene_grid_field") is not None
    assert avr_lib.avr_abi_version() == 2
