"""Particle fields without a GPU: the numpy reference (particle_reference) against numbers that are
known without it -- a particle at a cell centre, at a corner shared by eight cells, exact
conservation across a coarse-fine seam, the rerouted shares of a half-cell layer written out by
hand, the order of the additions, what is outside --, the refusals of api.deposit_scene and of the
registry that come before any device work, name collisions across the five registries, and the
declarations of the two native entries."""
import math
import os

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, particles
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds

import gradient_reference as ref
import particle_reference as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# one level of 4^3 unit cells; and the same with its upper half in x refined by two
FLAT_DOMAINS, FLAT_BOXES = [((0, 0, 0), (3, 3, 3))], [[((0, 0, 0), (3, 3, 3))]]
SEAM_DOMAINS = [((0, 0, 0), (3, 3, 3)), ((0, 0, 0), (7, 7, 7))]
SEAM_BOXES = [[((0, 0, 0), (3, 3, 3))], [((4, 0, 0), (7, 7, 7))]]
LO, HI = (0.0, 0.0, 0.0), (4.0, 4.0, 4.0)


def clear_registries():
    for names, remove in ((api.particle_fields, api.remove_particle_field),
                          (api.grid_fields, api.remove_grid_field),
                          (api.clump_fields, api.remove_clump_field),
                          (api.gradient_fields, api.remove_gradient_field),
                          (api.derived_fields, api.remove_field)):
        for name in list(names()):
            remove(name)


@pytest.fixture(autouse=True)
def _empty_registries():
    clear_registries()
    yield
    clear_registries()


def make(domains, boxes, ratio):
    levels = ref.make_levels(domains, boxes, ratio, 5)
    sizes = ref.cell_sizes(levels, LO, HI)
    return pr.hierarchy(levels, ratio, sizes, LO), sizes


@pytest.fixture(scope="module")
def flat():
    return make(FLAT_DOMAINS, FLAT_BOXES, [])[0]


@pytest.fixture(scope="module")
def seam():
    return make(SEAM_DOMAINS, SEAM_BOXES, [2])[0]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def put(h, points, values, method, quantity=pr.SUM):
    found = pr.contributions(h, np.array(points, dtype=np.float64), values, method)
    return found, pr.deposit(h, found, quantity)


# ---- the reference ---------------------------------------------------------------------------------

def test_a_particle_at_a_cell_centre_keeps_its_value_and_hands_out_seven_zero_shares(flat):
    found, dense = put(flat, [[1.5, 1.5, 1.5]], [3.0], pr.CIC)
    assert found["outside"] == 0 and found["rerouted"] == 0
    assert found["index"][0, 0].tolist() == [1, 1, 1] and found["index"][0, 7].tolist() == [2, 2, 2]
    assert np.array_equal(bits(found["shares"][0]), bits([3.0] + [0.0] * 7))
    want = np.zeros((4, 4, 4))
    want[1, 1, 1] = 3.0
    assert np.array_equal(bits(dense[0]), bits(want))
    # nearest grid point: one entry, the value's bits kept
    odd = float(np.array([0x7ff8000000001234], dtype=np.uint64).view(np.float64)[0])
    found, dense = put(flat, [[1.5, 1.5, 1.5], [0.1, 0.2, 3.9]], [-0.0, odd], pr.NGP)
    assert found["index"][:, 0].tolist() == [[1, 1, 1], [0, 0, 3]]
    assert np.array_equal(bits(found["shares"][:, 0]), bits([-0.0, odd]))
    assert bits(dense[0][1, 1, 1]) == bits(0.0)          # +0.0 + -0.0


def test_a_particle_at_a_corner_shared_by_eight_cells_gives_each_an_eighth(flat):
    found, dense = put(flat, [[2.0, 2.0, 2.0]], [8.0], pr.CIC)
    assert found["rerouted"] == 0
    want = np.zeros((4, 4, 4))
    want[1:3, 1:3, 1:3] = 1.0
    assert np.array_equal(bits(dense[0]), bits(want))
    # corner c = 4 dk + 2 dj + di
    assert found["index"][0, 1].tolist() == [2, 1, 1] and found["index"][0, 4].tolist() == [1, 1, 2]


@pytest.mark.parametrize("quantity", [pr.SUM, pr.DENSITY])
@pytest.mark.parametrize("method", [pr.NGP, pr.CIC])
def test_integer_values_on_quarter_cells_are_conserved_exactly_across_a_seam(seam, method,
                                                                             quantity):
    rng = np.random.default_rng(11)
    points = rng.integers(-2, 35, size=(500, 3)).astype(np.float64) / 8.0   # quarters of a fine cell
    points[:40, 0] = rng.integers(12, 21, size=40) / 8.0                    # around the seam at x = 2
    values = rng.integers(-50, 51, size=500).astype(np.float64)
    found, dense = put(seam, points, values, method, quantity)
    inside = found["leaf_level"] >= 0
    assert 0 < found["outside"] == int((~inside).sum()) < 500
    assert (found["leaf_level"] == 0).any() and (found["leaf_level"] == 1).any()
    total = 0.0
    for l, cells in enumerate(dense):
        volume = (seam.dx[l][0] * seam.dx[l][1]) * seam.dx[l][2]
        assert np.frexp(volume)[0] == 0.5
        total += float(cells.sum()) * (volume if quantity == pr.DENSITY else 1.0)
        assert not cells[~seam.mask[l]].any()            # nothing lands on a cell that is no leaf
    assert total == float(values[inside].sum())
    if method == pr.CIC:
        assert found["rerouted"] > 0


def test_the_rerouted_shares_of_a_half_cell_layer_stay_in_the_leaf(flat, seam):
    # a quarter of a cell from the domain's lower x face: the four corners with di = 0 lie at i = -1
    found, dense = put(flat, [[0.25, 1.5, 1.5]], [4.0], pr.CIC)
    assert found["rerouted"] == 4 and found["outside"] == 0
    assert found["shares"][0].tolist() == [1.0, 3.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert [found["index"][0, c].tolist() for c in (0, 1, 2, 3)] == \
        [[0, 1, 1], [0, 1, 1], [0, 1, 1], [0, 2, 1]]
    want = np.zeros((4, 4, 4))
    want[1, 1, 0] = 4.0
    assert np.array_equal(bits(dense[0]), bits(want))
    # the coarse side of the seam at x = 2: the corners with di = 1 name a coarse cell that finer
    # cells cover
    found, dense = put(seam, [[1.75, 1.5, 1.5]], [4.0], pr.CIC)
    assert found["leaf_level"].tolist() == [0] and found["rerouted"] == 4
    want = np.zeros((4, 4, 4))
    want[1, 1, 1] = 4.0
    assert np.array_equal(bits(dense[0]), bits(want)) and not dense[1].any()
    # the fine side: the corners with di = 0 fall to the coarse cell, which is there
    found, dense = put(seam, [[2.125, 1.75, 1.75]], [4.0], pr.CIC)
    assert found["leaf_level"].tolist() == [1] and found["rerouted"] == 0
    assert found["level"][0].tolist() == [0, 1, 0, 1, 0, 1, 0, 1]
    assert dense[0][1, 1, 1] == 1.0 and dense[1][3, 3, 4] == 3.0
    # a corner of the domain: seven of eight
    found, _ = put(flat, [[0.25, 0.25, 3.75]], None, pr.CIC)
    assert found["rerouted"] == 7


def test_a_cells_shares_are_added_in_list_order(flat):
    # nearest grid point anywhere in the cell; a cloud from the cell's centre, where the cell's
    # own weight is 1 and the others' 0
    for method, at in ((pr.NGP, [1.2, 2.7, 0.4]), (pr.CIC, [1.5, 2.5, 0.5])):
        _, dense = put(flat, [at] * 3, [1e16, 1.0, -1e16], method)
        assert dense[0][0, 2, 1] == 0.0
        _, dense = put(flat, [at] * 3, [1e16, -1e16, 1.0], method)
        assert dense[0][0, 2, 1] == 1.0


def test_what_is_outside_and_what_an_infinite_value_does(flat):
    nan, inf = math.nan, math.inf
    points = [[4.0, 1.0, 1.0], [1.0, 4.0, 1.0], [nan, 1.0, 1.0], [1.0, inf, 1.0], [1.0, 1.0, -inf],
              [1e300, 1.0, 1.0], [-0.001, 1.0, 1.0], [np.nextafter(4.0, 0.0), 1.0, 1.0]]
    for method in (pr.NGP, pr.CIC):
        found, dense = put(flat, points, None, method)
        assert found["leaf_level"].tolist() == [-1] * 7 + [0] and found["outside"] == 7
        assert (found["level"][:7] == -1).all() and not found["shares"][:7].any()
        assert found["leaf_index"][7].tolist() == [3, 1, 1] and dense[0][1, 1, 3] > 0.0
    found, dense = put(flat, [[1.5, 1.5, 1.5]], [inf], pr.CIC)
    assert dense[0][1, 1, 1] == inf
    assert np.isnan(dense[0][1:3, 1:3, 1:3]).sum() == 7 and np.isnan(dense[0]).sum() == 7


# ---- refusals before any device work -----------------------------------------------------------

class NoDevice:
    def __getattr__(self, name):
        raise AssertionError(f"the context was used ({name})")


def test_deposit_scene_refuses_other_ranks_and_wrong_arguments_before_device_work():
    box = AmrBox((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), level=0, dims=(4, 4, 4))
    bounds = VolumeBounds((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    full = api.SceneGeometry([box, box], [box, box], ScalarTransform(), bounds)
    part = api.SceneGeometry([box, box], [box], ScalarTransform(), bounds)
    at, v = np.zeros((5, 3)), np.ones(5)
    levels = ([(0.25, 0.25, 0.25)], (0.0, 0.0, 0.0), [])
    with pytest.raises(NotImplementedError):
        api.deposit_scene(NoDevice(), full, at, v, *levels, rank=0, n_ranks=2)
    with pytest.raises(NotImplementedError):
        api.deposit_scene(NoDevice(), part, at, v, *levels)
    wrong = [dict(positions=np.zeros((5, 2))), dict(positions=np.zeros(15)),
             dict(positions=np.zeros((5, 3), dtype=np.complex128)),
             dict(positions=np.zeros((5, 3), dtype=bool)), dict(values=np.ones(4)),
             dict(values=np.ones((5, 1))), dict(values=np.array(["a"] * 5)),
             dict(method="tsc"), dict(method=1), dict(quantity="mass"), dict(quantity=0)]
    for changed in wrong:
        a = {**dict(positions=at, values=v, method="cic", quantity="density"), **changed}
        with pytest.raises(ValueError):
            api.deposit_scene(NoDevice(), full, a["positions"], a["values"], *levels,
                              method=a["method"], quantity=a["quantity"])


def test_the_registry_checks_its_arguments_and_copies_the_arrays():
    at, v = np.zeros((5, 3)), np.arange(5.0)
    wrong = [lambda: api.add_particle_field("", at), lambda: api.add_particle_field(3, at),
             lambda: api.add_particle_field("stars", np.zeros((5, 4))),
             lambda: api.add_particle_field("stars", at, np.ones(6)),
             lambda: api.add_particle_field("stars", at.astype(np.complex64)),
             lambda: api.add_particle_field("stars", at, v, method="sph"),
             lambda: api.add_particle_field("stars", at, v, quantity="count")]
    for call in wrong:
        with pytest.raises(ValueError):
            call()
    for name in ("x", "cell_volume", "sqrt", "cells", "field"):
        with pytest.raises(ValueError, match="cannot name a particle field"):
            api.add_particle_field(name, at)
    assert api.particle_fields() == {}
    api.add_particle_field("stars", at, v.astype(np.float32), "ngp", "sum")
    api.add_particle_field("sinks", [[1, 2, 3]])
    found = api.particle_fields()
    assert list(found) == ["stars", "sinks"]
    assert found["stars"]["method"] == "ngp" and found["stars"]["quantity"] == "sum"
    assert found["sinks"]["method"] == "cic" and found["sinks"]["quantity"] == "density"
    assert found["sinks"]["values"] is None and found["sinks"]["positions"].dtype == np.float64
    at[0, 0], v[1] = 9.0, 9.0                            # the caller's arrays are its own again
    assert found["stars"]["positions"][0, 0] == 0.0 and found["stars"]["values"][1] == 1.0
    assert found["stars"]["values"].dtype == np.float64
    api.remove_particle_field("sinks")
    assert list(api.particle_fields()) == ["stars"]
    with pytest.raises(KeyError):
        api.remove_particle_field("sinks")
    assert particles.METHODS == ("ngp", "cic") and particles.QUANTITIES == ("sum", "density")


def test_a_name_belongs_to_one_of_the_five_registries_and_a_particle_field_is_a_leaf():
    from amrvolumerenderer_amd import gradient
    adders = {"derived": lambda n: api.add_field(n, "u * 2"),
              "gradient": lambda n: api.add_gradient_field(n, "u", "x"),
              "clump": lambda n: api.add_clump_field(n, "u", 0.0),
              "grid": lambda n: api.add_array_field(n, np.zeros((2, 2, 2)), 0),
              "particle": lambda n: api.add_particle_field(n, np.zeros((1, 3)))}
    for first, add in adders.items():
        add("taken")
        for second, again in adders.items():
            if first != second:
                with pytest.raises(ValueError, match="is a registered"):
                    again("taken")
        clear_registries()
    # a leaf of the graph: read by the others, reading none, so no cycle can pass through it
    api.add_particle_field("stars", np.zeros((1, 3)))
    api.add_field("rho_all", "u + stars")
    api.add_potential_field("phi", "rho_all")
    api.add_gradient_field("dstars", "stars", "x")
    assert gradient._dependencies("stars", api.derived_fields(), api.gradient_fields(),
                                  api.clump_fields()) == ()
    assert "stars" in gradient._dependencies("rho_all", api.derived_fields(),
                                             api.gradient_fields(), api.clump_fields())


def test_a_plotfile_level_call_takes_a_particle_field_without_asking_the_plotfile_for_it(
        tmp_path, monkeypatch):
    from amrvolumerenderer_amd import plotfile
    levels = ref.make_levels(FLAT_DOMAINS, FLAT_BOXES, [], 5)
    path = str(tmp_path / "plt")
    plotfile.write_plotfile(path, list(ref.VARIABLES), levels, LO, HI, [])

    def untouched(*args, **kwargs):
        raise AssertionError("the runtime was touched")

    monkeypatch.setattr(api, "_runtime_scope", untouched)
    monkeypatch.setattr(api, "_ensure_runtime", untouched)
    monkeypatch.setattr(api, "_load_variable_scenes", untouched)
    api.add_particle_field("stars", np.zeros((1, 3)))
    api.add_field("both", "u + stars")
    api.add_field("broken", "missing + stars")
    for name in ("stars", "both"):
        with pytest.raises(AssertionError, match="the runtime was touched"):
            api.covering_grid(path, 0, [name])
    with pytest.raises(RuntimeError, match="not found in plotfile"):
        api.covering_grid(path, 0, ["broken"])


# ---- declarations ------------------------------------------------------------------------------------

def test_the_entries_are_declared_and_exported(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    assert "int avr_scene_particle_cells(avr_context *ctx, const avr_scene *scene, " \
           "const double *points_dev" in header
    assert "int avr_scene_particle_deposit(avr_context *ctx, avr_scene *out, " \
           "const int64_t *cells_sorted_dev" in header
    for entry, count in (("avr_scene_particle_cells", 15), ("avr_scene_particle_deposit", 8)):
        declared = header.split(f"int {entry}(")[1].split(");")[0]
        assert len(_capi.SIGNATURES[entry][1]) == declared.count(",") + 1 == count
        assert getattr(avr_lib, entry) is not None
    assert avr_lib.avr_abi_version() == 2
