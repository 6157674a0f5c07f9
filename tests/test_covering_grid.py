"""Covering grids without a GPU: the numpy reference (covering_grid_reference) against numbers that
are known without it -- the classes of cells of the three-level fixture, exact conservation of an
integer field --, grids.index_region, grid_edges and the .npz file, the refusals of
api.covering_grid and api.covering_grid_scene that come before any device work, and the
declarations of the native entry."""
import math
import os

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, grids, plotfile
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds

import covering_grid_reference as cg
import gradient_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIABLES = list(ref.VARIABLES)

THREE_DOMAINS = [((0, 0, 0), (11, 5, 7)), ((0, 0, 0), (23, 11, 15)), ((0, 0, 0), (47, 23, 31))]
# two fine boxes that touch at i = 11 | 12; the finest grid lies inside the first
THREE_BOXES = [[((0, 0, 0), (6, 5, 7)), ((7, 0, 0), (11, 5, 7))],
               [((4, 2, 2), (11, 7, 9)), ((12, 2, 2), (17, 9, 9))],
               [((12, 6, 6), (21, 13, 15))]]
THREE_LO, THREE_HI, THREE_RATIO = (0.0, -1.0, 2.0), (1.5, 0.5, 3.0), [2, 2]


@pytest.fixture(scope="module")
def three():
    return ref.make_levels(THREE_DOMAINS, THREE_BOXES, THREE_RATIO, 71)


def whole(levels, level, variable="u", **load):
    lo, dims = cg.whole_domain(levels, THREE_RATIO, level)
    return cg.covering_grid(levels, THREE_RATIO, VARIABLES.index(variable), level, lo, dims, **load)


def coverages(result):
    found, counts = np.unique(result["coverage"], return_counts=True)
    return dict(zip(found.tolist(), counts.tolist()))


# ---- the reference ---------------------------------------------------------------------------------

@pytest.mark.parametrize("level, counts", [(0, {0: 480, 1: 69, 2: 27}),
                                           (1, {0: 3840, 1: 668, 2: 100}),
                                           (2, {0: 30720, 1: 5344, 2: 800})])
def test_all_levels_loaded_every_cell_is_covered_once_and_no_covered_cell_is_read(three, level,
                                                                                  counts):
    got = whole(three, level)
    assert cg.class_counts(got) == counts
    assert coverages(got) == {1.0: sum(counts.values())}
    assert not (np.abs(got["values"]) >= 1e29).any()            # the poison under finer grids
    mixed = int((got["levels_used"] == 2).sum())
    assert mixed == (23 if level == 0 else 0)                   # of the 96 averaged cells
    assert int((got["levels_used"] >= 1).sum()) == got["values"].size
    if level == 0:
        assert int((got["level"] > 0).sum()) == 96


def test_level_cuts_leave_absent_and_partly_covered_cells(three):
    finest_only = whole(three, 0, min_level=2)
    assert cg.class_counts(finest_only) == {-1: 549, 2: 27}
    assert coverages(finest_only) == {0.0: 549, 0.125: 2, 0.25: 9, 0.5: 12, 1.0: 4}
    assert np.isnan(finest_only["values"][finest_only["level"] < 0]).all()
    upper = whole(three, 0, min_level=1)
    assert cg.class_counts(upper) == {-1: 480, 1: 69, 2: 27}
    assert coverages(upper) == {0.0: 480, 1.0: 96}
    coarse = whole(three, 1, max_level=0)
    assert cg.class_counts(coarse) == {0: 4608} and coverages(coarse) == {1.0: 4608}
    finer_than_loaded = whole(three, 2, max_level=1)
    assert cg.class_counts(finer_than_loaded) == {0: 30720, 1: 6144}


def test_a_coarser_leaf_is_repeated_and_a_same_level_leaf_is_copied_by_bits(three):
    got = whole(three, 2, "odd")
    arrays, _ = ref.leaf_arrays(three, THREE_RATIO, VARIABLES.index("odd"))
    for level, (origin, mask, values) in enumerate(arrays):
        up = 2 ** (2 - level)
        dense = np.repeat(np.repeat(np.repeat(values, up, 0), up, 1), up, 2)
        at = np.repeat(np.repeat(np.repeat(mask, up, 0), up, 1), up, 2)
        assert ref.same_bits(got["values"][at], dense[at])
        assert (got["level"][at] == level).all()
    assert np.isnan(got["values"]).any() and np.isinf(got["values"]).any()


def test_the_fill_value_keeps_its_bits(three):
    payload = float(np.array([0x7ff8000000001234], dtype=np.uint64).view(np.float64)[0])
    for fill in (-0.0, payload, 7.5):
        got = whole(three, 0, min_level=2, fill=fill)
        absent = got["values"][got["level"] < 0]
        assert (absent.view(np.uint64) == np.array([fill]).view(np.uint64)[0]).all()


def test_an_integer_field_is_conserved_exactly(three):
    """sum(value * coverage) * R^3 over the level-0 grid against the sum over the leaves of v *
    (finest cells per leaf): the weights are powers of two and the values integers of at most
    1000, so every term and every partial sum is an integer far below 2^53."""
    got = whole(three, 0, "whole")
    arrays, _ = ref.leaf_arrays(three, THREE_RATIO, VARIABLES.index("whole"))
    finest_per_leaf = [64.0, 8.0, 1.0]
    want = sum(float(values[mask].sum()) * cells
               for (_, mask, values), cells in zip(arrays, finest_per_leaf))
    total = float((got["values"] * got["coverage"]).sum()) * 64.0
    print("conserved:", total, "leaves:", want)
    assert total == want and want == math.floor(want) and abs(want) < 2.0 ** 53
    # ... and cell by cell at level 1
    finer = whole(three, 1, "whole")
    assert float((finer["values"] * finer["coverage"]).sum()) * 8.0 == want


def test_a_region_past_the_domain_and_below_zero(three):
    inner = whole(three, 1)
    got = cg.covering_grid(three, THREE_RATIO, 0, 1, (-3, -2, -1), (30, 16, 19))
    assert ref.same_bits(got["values"][1:17, 2:14, 3:27], inner["values"])
    outside = np.ones(got["values"].shape, dtype=bool)
    outside[1:17, 2:14, 3:27] = False
    assert (got["level"][outside] == -1).all() and (got["coverage"][outside] == 0.0).all()
    assert np.isnan(got["values"][outside]).all()


# ---- grids -----------------------------------------------------------------------------------------

def test_index_region_on_faces_inside_cells_outside_the_domain_and_below_prob_lo():
    prob_lo, size = (0.0, -1.0, 2.0), (0.125, 0.25, 0.0625)
    # faces: cells 2 .. 5, 0 .. 3, 4 .. 4
    assert grids.index_region(prob_lo, size, (0.25, -1.0, 2.25), (0.75, 0.0, 2.3125)) == \
        ((2, 0, 4), (4, 4, 1))
    # inside cells: a cell is in exactly when its centre is in [left, right)
    assert grids.index_region(prob_lo, size, (0.26, -0.9, 2.0), (0.60, -0.1, 2.04)) == \
        ((2, 0, 0), (3, 4, 1))                 # centres 0.3125 .. 0.5625 | -0.875 .. -0.125 | 2.03125
    assert grids.index_region(prob_lo, size, (0.3125, -0.875, 2.0), (0.5625, -0.125, 2.1)) == \
        ((2, 0, 0), (2, 3, 2))                 # a centre on the left edge is in, on the right out
    # past the domain and below prob_lo
    lo, dims = grids.index_region(prob_lo, size, (-0.5, -2.0, 1.9), (100.0, -1.5, 2.0))
    assert lo == (-4, -4, -2) and dims == (804, 2, 2)
    left, right = grids.grid_edges(prob_lo, size, lo, dims)
    assert left == (-0.5, -2.0, 1.875) and right == (100.0, -1.5, 2.0)
    # a size that is no power of two: the centres themselves decide
    third = (1.0 / 3.0,) * 3
    lo, dims = grids.index_region((0.0,) * 3, third, (0.5,) * 3, (2.5,) * 3)
    assert lo == (1, 1, 1) and dims == (6, 6, 6)          # centres 0.5 (in) .. 2.1666, 2.5 out
    for wrong in (dict(left_edge=(0.3, 0.0, 2.0), right_edge=(0.3, 1.0, 3.0)),       # empty
                  dict(left_edge=(0.26, 0.0, 2.0), right_edge=(0.30, 1.0, 3.0)),     # no centre
                  dict(left_edge=(0.5, 0.0, 2.0), right_edge=(0.25, 1.0, 3.0)),      # reversed
                  dict(left_edge=(math.nan, 0.0, 2.0), right_edge=(1.0, 1.0, 3.0)),
                  dict(left_edge=(0.0, 0.0, 2.0), right_edge=(math.inf, 1.0, 3.0)),
                  dict(left_edge=(0.0, 0.0), right_edge=(1.0, 1.0, 3.0)),
                  dict(left_edge=(-1e12, 0.0, 2.0), right_edge=(1.0, 1.0, 3.0))):
        with pytest.raises(ValueError):
            grids.index_region(prob_lo, size, **wrong)
    with pytest.raises(ValueError):
        grids.index_region(prob_lo, (0.125, 0.0, 0.25), (0.0, 0.0, 2.0), (1.0, 1.0, 3.0))


def test_an_npz_file_gives_back_what_was_saved(tmp_path, three):
    got = cg.covering_grid(three, THREE_RATIO, 1, 0, (-1, 0, 0), (5, 3, 2), min_level=1)
    grid = {"level": 0, "lo": (-1, 0, 0), "dims": (5, 3, 2), "left_edge": (-0.125, -1.0, 2.0),
            "right_edge": (0.5, -0.25, 2.25), "cell_size": (0.125, 0.25, 0.125),
            "fields": {"odd": got["values"], "x velocity": got["coverage"]},
            "coverage": got["coverage"], "cell_level": got["level"], "absent": 30, "partial": 0}
    path = str(tmp_path / "grid.npz")
    grids.save_npz(grid, path)
    assert os.path.exists(path) and not os.path.exists(path + ".npz")
    back = grids.load_npz(path)
    assert set(back) == set(grid) and list(back["fields"]) == ["odd", "x velocity"]
    for key in ("level", "lo", "dims", "left_edge", "right_edge", "cell_size", "absent", "partial"):
        assert back[key] == grid[key], key
    assert ref.same_bits(back["fields"]["odd"], got["values"])
    assert ref.same_bits(back["coverage"], got["coverage"])
    assert back["cell_level"].dtype == np.int8 and np.array_equal(back["cell_level"], got["level"])
    with np.load(path) as raw:
        assert "fields/odd" in raw.files and "coverage" in raw.files


# ---- refusals before any device work -----------------------------------------------------------

def test_api_covering_grid_refuses_wrong_arguments_before_anything_is_loaded(tmp_path, monkeypatch,
                                                                             three):
    path = str(tmp_path / "plt")
    plotfile.write_plotfile(path, VARIABLES, three, THREE_LO, THREE_HI, THREE_RATIO)

    def untouched(*args, **kwargs):
        raise AssertionError("the runtime was touched")

    monkeypatch.setattr(api, "_runtime_scope", untouched)
    monkeypatch.setattr(api, "_ensure_runtime", untouched)
    monkeypatch.setattr(api, "_load_variable_scenes", untouched)
    region = ((0, 0, 0), (3, 3, 3))
    edges = dict(left_edge=(0.0, -1.0, 2.0), right_edge=(0.5, 0.0, 2.5))
    wrong = [dict(region=region, **edges), dict(region=region, left_edge=edges["left_edge"]),
             dict(region=region, right_edge=edges["right_edge"]),
             dict(left_edge=edges["left_edge"]), dict(right_edge=edges["right_edge"]),
             dict(region=((0, 0, 0), (3, -1, 3))),                      # dims of 0 along y
             dict(region=((4, 0, 0), (2, 3, 3))), dict(region=((0, 0), (3, 3))),
             dict(left_edge=(0.3, -1.0, 2.0), right_edge=(0.3, 0.0, 2.5)),   # holds no centre
             dict(level=-1), dict(level=3), dict(level=2, max_level=1, region=((0, 0, 0), (3, 3, -1)))]
    for arguments in wrong:
        with pytest.raises(ValueError):
            api.covering_grid(path, **arguments)
    with pytest.raises(RuntimeError):
        api.covering_grid(str(tmp_path / "none"))
    with pytest.raises(RuntimeError):
        api.covering_grid(path, fields=["no such field"])
    # ... and what is in order reaches the loader: a level finer than the loaded ones too
    for arguments in (dict(), dict(level=2, max_level=0), dict(level=0, region=region), edges):
        with pytest.raises(AssertionError, match="the runtime was touched"):
            api.covering_grid(path, **arguments)


def test_boxes_on_other_ranks_and_wrong_arguments_are_refused_before_device_work():
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"the context was used ({name})")

    box = AmrBox((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), level=0, dims=(4, 4, 4))
    bounds = VolumeBounds((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    full = api.SceneGeometry([box, box], [box, box], ScalarTransform(), bounds)
    part = api.SceneGeometry([box, box], [box], ScalarTransform(), bounds)
    arguments = ((0, 0, 0), (4, 4, 4), [(0.25, 0.25, 0.25)], (0.0, 0.0, 0.0), [])
    with pytest.raises(NotImplementedError):
        api.covering_grid_scene(NoDevice(), full, 0, *arguments, rank=0, n_ranks=2)
    with pytest.raises(NotImplementedError):
        api.covering_grid_scene(NoDevice(), part, 0, *arguments)
    for level, lo, dims in ((0, (0, 0, 0), (4, 0, 4)), (0, (0, 0), (4, 4, 4)), (1, (0, 0, 0), (4, 4, 4)),
                            (-1, (0, 0, 0), (4, 4, 4))):
        with pytest.raises(ValueError):
            api.covering_grid_scene(NoDevice(), full, level, lo, dims, *arguments[2:])


# ---- declarations ------------------------------------------------------------------------------------

def test_the_entry_is_declared_and_exported(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    assert "int avr_scene_covering_grid(avr_context *ctx, const avr_scene *field, int level" in header
    declared = header.split("int avr_scene_covering_grid(")[1].split(");")[0]
    assert len(_capi.SIGNATURES["avr_scene_covering_grid"][1]) == declared.count(",") + 1 == 12
    assert getattr(avr_lib, "avr_scene_covering_grid") is not None
    assert avr_lib.avr_abi_version() == 2
