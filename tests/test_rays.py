"""Rays without a GPU: the reference (ray_reference) against things that are not its twin -- the
tiling of a ray by its segments, every segment's midpoint located by the streamlines' leaf rule,
axis rays against the covering grid's column and the on-axis projection's column sum, the diagonal
of a uniform grid, rays on faces, one ray of every status, holes -- and the host side of the API:
rays.py, the declared ABI entry, api.rays and api.ray_scene with the device work patched out."""
import math
import os
import types

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, plotfile
from amrvolumerenderer_amd import rays as ray_rules
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds

import axis_projection_reference as axis_ref
import covering_grid_reference as grid_ref
import gradient_reference as ref
import ray_reference as rr
import streamline_reference as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52

THREE_DOMAINS = [((0, 0, 0), (11, 5, 7)), ((0, 0, 0), (23, 11, 15)), ((0, 0, 0), (47, 23, 31))]
# two fine boxes that touch at i = 11 | 12; the finest grid lies inside the first
THREE_BOXES = [[((0, 0, 0), (6, 5, 7)), ((7, 0, 0), (11, 5, 7))],
               [((4, 2, 2), (11, 7, 9)), ((12, 2, 2), (17, 9, 9))],
               [((12, 6, 6), (21, 13, 15))]]
THREE_LO, THREE_HI = (0.0, -1.0, 2.0), (1.5, 0.5, 3.0)


class Case:
    def __init__(self, domains, boxes, lo, hi, ratio, seed):
        self.levels = ref.make_levels(domains, boxes, ratio, seed)
        self.lo, self.hi, self.ratio = lo, hi, list(ratio)
        self.sizes = ref.cell_sizes(self.levels, lo, hi)
        for size in self.sizes:
            assert all(np.frexp(s)[0] == 0.5 for s in size)         # powers of two
        self.cache = {}

    def hierarchy(self, component=0, min_level=0, max_level=-1):
        key = (component, min_level, max_level)
        if key not in self.cache:
            self.cache[key] = rr.Hierarchy(self.levels, self.ratio, component, self.sizes, self.lo,
                                           min_level, max_level)
        return self.cache[key]

    def locator(self, component=0, min_level=0, max_level=-1):
        """The streamlines' reference: its leaf rule locates points independently."""
        key = ("sl", component, min_level, max_level)
        if key not in self.cache:
            self.cache[key] = sl.Hierarchy(self.levels, self.ratio, (component,) * 3, self.sizes,
                                           self.lo, min_level, max_level)
        return self.cache[key]


@pytest.fixture(scope="module")
def three():
    return Case(THREE_DOMAINS, THREE_BOXES, THREE_LO, THREE_HI, [2, 2], 81)


def generic_rays(case, n, seed, margin=0.2):
    """n rays between points spread over the domain grown by `margin` of its size: the end points
    are products of irrational-looking numbers, so no ray runs along a face or through an edge."""
    lo, hi = np.array(case.lo), np.array(case.hi)
    s = np.arange(1, n + 1, dtype=np.float64)[:, None] + seed
    fa = np.mod(s * np.array([math.sqrt(2.0), math.sqrt(3.0), math.sqrt(5.0)]), 1.0)
    fb = np.mod(s * np.array([math.sqrt(7.0), math.sqrt(11.0), math.sqrt(13.0)]) + 0.37, 1.0)
    grow = lambda f: lo + (f * (1.0 + 2.0 * margin) - margin) * (hi - lo)
    return grow(fa), grow(fb)


def per_ray(out):
    offsets = out["offsets"]
    return [slice(int(offsets[s]), int(offsets[s + 1])) for s in range(offsets.size - 1)]


def check_tiling(out):
    """t0[0] == t_enter, t1[i] == t0[i + 1] and t1 > t0, by bits."""
    for s, cut in enumerate(per_ray(out)):
        t0, t1 = out["t0"][cut], out["t1"][cut]
        if out["status"][s] in (rr.MISS, rr.INVALID):
            assert t0.size == 0 and math.isnan(out["t_enter"][s]) and math.isnan(out["t_leave"][s])
            continue
        assert (t1 > t0).all()
        if t0.size:
            assert t0[0] == out["t_enter"][s]
            assert np.array_equal(t1[:-1].view(np.uint64), t0[1:].view(np.uint64))
            assert t1[-1] <= out["t_leave"][s]


def check_midpoints(case, out, start, end, locator, share=0.02):
    """Every segment longer than 1e-9: its midpoint, located by the streamlines' leaf rule, lies
    in a leaf of the recorded level that holds the recorded value bits (level -1: in no leaf)."""
    ray = np.repeat(np.arange(out["offsets"].size - 1), np.diff(out["offsets"]))
    long_enough = out["t1"] - out["t0"] > 1e-9
    total = out["t0"].size
    assert total > 0 and (~long_enough).sum() <= share * total
    t = 0.5 * (out["t0"] + out["t1"])
    points = start[ray] + t[:, None] * (end[ray] - start[ray])
    level, _, index = locator.locate(points)
    assert np.array_equal(level[long_enough], out["level"][long_enough].astype(np.int64))
    for l in range(locator.max_level + 1):
        pick = long_enough & (level == l)
        is_leaf, at = locator.leaf(l, index[pick])
        assert is_leaf.all()
        assert ref.same_bits(locator.values[l][0][at], out["value"][pick])
    assert np.isnan(out["value"][out["level"] < 0]).all()
    return int((~long_enough).sum()), total


# ---- tiling and midpoints ------------------------------------------------------------------------

def test_segments_tile_the_ray_and_their_midpoints_lie_in_the_recorded_leaves(three):
    start, end = generic_rays(three, 150, 0.0)
    hierarchy = three.hierarchy()
    out = hierarchy.rays(start, end, hierarchy.default_max_trips())
    check_tiling(out)
    short, total = check_midpoints(three, out, start, end, three.locator())
    print("segments:", total, "shorter than 1e-9:", short)
    status = out["status"]
    assert (status == rr.COMPLETE).sum() > 100 and (status == rr.TRUNCATED).sum() == 0
    assert set(out["level"].tolist()) == {0, 1, 2}            # the box domain is fully covered
    # a complete ray ends at t_leave to 4 ulp
    for s, cut in enumerate(per_ray(out)):
        if status[s] == rr.COMPLETE:
            last, leave = out["t1"][cut][-1], out["t_leave"][s]
            assert abs(last - leave) <= 4 * np.spacing(leave)
    # covered: every ray lies in leaves from t_enter to t_leave
    d = end - start
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    inside = status == rr.COMPLETE
    counts = np.diff(out["offsets"])
    span = (out["t_leave"] - out["t_enter"]) * length
    assert (np.abs(out["covered"] - span)[inside] <= 4 * EPS * (counts * span)[inside]).all()


# ---- axis rays -----------------------------------------------------------------------------------

AXIS_LO, AXIS_HI = (0.0, 0.0, 0.0), (2.0, 1.0, 1.0)
# ratios, the level domains, the grids (the finest inside the middle one), a finest cell inside
AXIS_CASES = {
    "2-2": ([2, 2], [((0, 0, 0), (7, 3, 3)), ((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))],
            [[((0, 0, 0), (7, 3, 3))], [((4, 2, 2), (11, 5, 5))], [((12, 6, 6), (19, 9, 9))]],
            [15, 7, 6]),
    "2-4": ([2, 4], [((0, 0, 0), (7, 3, 3)), ((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (63, 31, 31))],
            [[((0, 0, 0), (7, 3, 3))], [((4, 2, 2), (11, 5, 5))], [((24, 12, 12), (39, 19, 19))]],
            [30, 14, 13]),
}


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("ratios", ["2-2", "2-4"])
def test_an_axis_ray_is_the_covering_grids_column_and_the_on_axis_projections_sum(ratios, axis):
    """A ray along the axis through the centres of a finest-level column that crosses all three
    levels.  Domain extents and cell sizes are powers of two, so every T is exact.  The integral
    is held against the covering grid's column in both cases; the on-axis projection's reference
    knows ratio 2 only, so its column is compared as well where both ratios are 2."""
    ratio, domains, boxes, fine = AXIS_CASES[ratios]
    case = Case(domains, boxes, AXIS_LO, AXIS_HI, ratio, 82)
    centre = [AXIS_LO[d] + (fine[d] + 0.5) * case.sizes[2][d] for d in range(3)]
    a, b = list(centre), list(centre)
    a[axis], b[axis] = AXIS_LO[axis], AXIS_HI[axis]
    hierarchy = case.hierarchy()
    out = hierarchy.rays([a], [b], hierarchy.default_max_trips())
    check_tiling(out)
    assert out["status"].tolist() == [rr.COMPLETE]
    assert out["t_enter"][0] == 0.0 and out["t_leave"][0] == 1.0 and out["t1"][-1] == 1.0
    # the covering grid's finest-level column, equal-leaf runs merged
    n = domains[2][1][axis] + 1
    lo, dims = list(fine), [1, 1, 1]
    lo[axis], dims[axis] = 0, n
    grid = grid_ref.covering_grid(case.levels, case.ratio, 0, 2, lo, dims)
    values, levels = grid["values"].reshape(-1), grid["level"].reshape(-1).astype(np.int64)
    refine = {0: ratio[0] * ratio[1], 1: ratio[1], 2: 1}
    leaf = [(int(l), i // refine[int(l)]) for i, l in enumerate(levels)]
    first = [i for i in range(n) if i == 0 or leaf[i] != leaf[i - 1]]
    assert ref.same_bits(out["value"], values[first])
    assert out["level"].tolist() == levels[first].tolist() and set(levels.tolist()) == {0, 1, 2}
    # the lengths are the cell sizes, by bits
    extent = AXIS_HI[axis] - AXIS_LO[axis]
    lengths = (out["t1"] - out["t0"]) * extent
    assert lengths.tolist() == [case.sizes[int(l)][axis] for l in out["level"]]
    assert out["covered"][0] == extent
    # the column integral, whatever the ratios: the covering grid's finest cells, each dx of the
    # finest level long, hold the ray's leaves, so their exact sum is the on-axis column
    count = out["t0"].size
    assert (levels >= 0).all() and np.isfinite(values).all()
    terms = (values * case.sizes[2][axis]).tolist()            # a power of two: exact products
    column, column_abs = math.fsum(terms), math.fsum(abs(t) for t in terms)
    print("integral:", out["integral"][0], "column:", column, "bound:", count * EPS * column_abs)
    assert abs(out["integral"][0] - column) <= count * EPS * column_abs
    if ratio != [2, 2]:
        return
    # the on-axis projection's column
    want = axis_ref.reference(case.levels, AXIS_LO, AXIS_HI, axis, 0, None, centre,
                              (1.0, 1.0), 1, 1, [size[axis] for size in case.sizes],
                              with_fsum=True)
    assert want["count"][0, 0] == count
    bound = count * EPS * want["integral_abs"][0, 0]
    print("integral:", out["integral"][0], "projection:", want["integral_fsum"][0, 0], "bound:", bound)
    assert abs(out["integral"][0] - want["integral_fsum"][0, 0]) <= bound


# ---- the diagonal of a uniform grid --------------------------------------------------------------

def test_the_corner_diagonal_of_a_uniform_grid_crosses_the_cells_i_i_i():
    n = 8
    domain = ((0, 0, 0), (n - 1, n - 1, n - 1))
    case = Case([domain], [[domain]], (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), [], 83)
    hierarchy = case.hierarchy()
    cells = case.levels[0]["data"][0][0]
    ahead = hierarchy.rays([[0.0, 0.0, 0.0]], [[1.0, 1.0, 1.0]], 100)
    back = hierarchy.rays([[1.0, 1.0, 1.0]], [[0.0, 0.0, 0.0]], 100)
    for out, order in ((ahead, range(n)), (back, range(n - 1, -1, -1))):
        check_tiling(out)
        assert out["status"].tolist() == [rr.COMPLETE] and out["offsets"].tolist() == [0, n]
        assert ref.same_bits(out["value"], [cells[i, i, i] for i in order])
        lengths = out["t1"] - out["t0"]
        assert (lengths == 0.125).all() and (out["level"] == 0).all()
    # the edge and corner cells between two diagonal cells took trips and emitted nothing
    assert hierarchy.rays([[0.0, 0.0, 0.0]], [[1.0, 1.0, 1.0]], 3 * n - 3)["status"].tolist() == [2]
    assert hierarchy.rays([[0.0, 0.0, 0.0]], [[1.0, 1.0, 1.0]], 3 * n - 2)["status"].tolist() == [0]


# ---- rays on faces -------------------------------------------------------------------------------

def test_a_ray_on_a_box_face_takes_the_cells_above_it(three):
    """y = -0.75 is the low face of the level-1 grid (j = 2 of level 1, the face between j = 0 and
    j = 1 of level 0), and z = 2.125 the low z face of the same grid (k = 2): a ray along x in both
    planes has D[1] == D[2] == 0 and takes the cells floor gives, those above the faces -- the
    fine cells over the grid's x range, never the coarse cells below."""
    a, b = [-0.25, -0.75, 2.125], [1.75, -0.75, 2.125]
    hierarchy = three.hierarchy()
    out = hierarchy.rays([a], [b], hierarchy.default_max_trips())
    check_tiling(out)
    assert out["status"].tolist() == [rr.COMPLETE]
    check_midpoints(three, out, np.array([a]), np.array([b]), three.locator(), share=0.0)
    middle = a[0] + 0.5 * (out["t0"] + out["t1"]) * (b[0] - a[0])
    over_grid = (middle > 0.25) & (middle < 1.125)          # level-1 cells i = 4 .. 17
    assert over_grid.sum() >= 14 and (out["level"][over_grid] == 1).all()
    assert (out["level"][~over_grid] == 0).all()
    # the same line just below the face runs through coarse cells only
    below = hierarchy.rays([[a[0], -0.75 - 2.0 ** -20, a[2]]], [[b[0], -0.75 - 2.0 ** -20, b[2]]],
                           hierarchy.default_max_trips())
    assert (below["level"] == 0).all() and below["offsets"].tolist() == [0, 12]
    # on the domain's high face a ray misses; on its low face it is inside
    assert hierarchy.rays([[-1.0, 0.5, 2.5]], [[2.0, 0.5, 2.5]], 100)["status"].tolist() == [rr.MISS]
    low = hierarchy.rays([[-1.0, -1.0, 2.0]], [[2.0, -1.0, 2.0]], 100)
    assert low["status"].tolist() == [rr.COMPLETE] and low["offsets"].tolist() == [0, 12]


# ---- one ray of every status ---------------------------------------------------------------------

def test_one_ray_of_every_status(three):
    hierarchy = three.hierarchy()
    inside, other = [0.3, -0.4, 2.3], [1.2, 0.3, 2.9]
    start = [[-1.0, -2.0, 2.5], [2.0, 0.0, 2.5],              # passes beside the domain; outside
             inside, [math.nan, 0.0, 2.5], inside,            # A == B, NaN, an infinite end point
             inside]                                          # in order
    end = [[-0.5, 1.0, 2.5], [3.0, 0.1, 2.6], inside, other, [math.inf, 0.3, 2.9], other]
    out = hierarchy.rays(start, end, hierarchy.default_max_trips())
    check_tiling(out)
    assert out["status"].tolist() == [1, 1, 3, 3, 3, 0]
    assert np.diff(out["offsets"])[:5].tolist() == [0] * 5 and np.diff(out["offsets"])[5] > 10
    assert (out["integral"][:5] == 0.0).all() and (out["covered"][:5] == 0.0).all()
    short = hierarchy.rays([inside], [other], 3)
    check_tiling(short)
    assert short["status"].tolist() == [rr.TRUNCATED] and 1 <= short["t0"].size <= 3
    whole = per_ray(out)[5]
    for key in ("t0", "t1", "level", "value"):
        assert ref.same_bits(short[key], out[key][whole][:short["t0"].size])


def test_rays_that_start_or_end_outside_have_the_clipped_span(three):
    hierarchy = three.hierarchy()
    inside, outside = [0.3, -0.4, 2.3], [-0.45, -0.4, 2.3]    # 0.75 apart along x, the face at 0.0
    out = hierarchy.rays([outside, inside, inside], [inside, outside, [0.7, 0.1, 2.6]], 1000)
    check_tiling(out)
    assert out["status"].tolist() == [0, 0, 0]
    assert out["t_enter"].tolist() == [0.45 / 0.75, 0.0, 0.0]
    assert out["t_leave"].tolist() == [1.0, (0.0 - 0.3) / (-0.45 - 0.3), 1.0]
    cuts = per_ray(out)
    assert out["t0"][cuts[0]][0] == out["t_enter"][0] and out["t1"][cuts[0]][-1] == 1.0
    assert out["t0"][cuts[1]][0] == 0.0 and out["t1"][cuts[1]][-1] == out["t_leave"][1]
    # the same cells, met in the opposite order
    assert ref.same_bits(out["value"][cuts[0]], out["value"][cuts[1]][::-1])


# ---- holes ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("min_level,max_level", [(1, -1), (0, 1), (1, 1)])
def test_level_cuts_leave_absent_stretches(three, min_level, max_level):
    start, end = generic_rays(three, 60, 0.5)
    hierarchy = three.hierarchy(0, min_level, max_level)
    out = hierarchy.rays(start, end, hierarchy.default_max_trips())
    check_tiling(out)
    check_midpoints(three, out, start, end, three.locator(0, min_level, max_level))
    absent = out["level"] < 0
    top = 2 if max_level < 0 else max_level
    assert set(out["level"][~absent].tolist()) == set(range(min_level, top + 1))
    if min_level == 1:
        # the hull of the two level-1 grids has a hole: i = 4 .. 11, j = 8 .. 9 of level 1
        assert absent.sum() > 10 and np.isnan(out["value"][absent]).all()
    else:
        assert not absent.any()                               # level 0 covers what level 2 did
    d = end - start
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    for s, cut in enumerate(per_ray(out)):
        if out["status"][s] != rr.COMPLETE:
            continue
        w = (out["t1"][cut] - out["t0"][cut]) * length[s]
        hole = out["level"][cut] < 0
        value = out["value"][cut]
        count = w.size
        span = (out["t_leave"][s] - out["t_enter"][s]) * length[s]
        assert abs(math.fsum(w[~hole]) - out["covered"][s]) <= count * EPS * span
        assert abs(out["covered"][s] + math.fsum(w[hole]) - span) <= 4 * count * EPS * span
        terms = (value * w)[~hole & np.isfinite(value)]
        assert abs(math.fsum(terms) - out["integral"][s]) <= count * EPS * np.abs(terms).sum()


# ---- rays.py -------------------------------------------------------------------------------------

def _result(n_fields=2):
    rng = np.random.default_rng(5)
    offsets = np.array([0, 3, 3, 7], dtype=np.int64)
    t0 = rng.random(7)
    fields = {name: rng.standard_normal(7) for name in ("density", "odd one")[:n_fields]}
    fields["density"][2] = math.nan
    return {"n": 3, "start": rng.standard_normal((3, 3)), "end": rng.standard_normal((3, 3)),
            "offsets": offsets, "status": np.array([0, 1, 2], dtype=np.uint8),
            "t_enter": np.array([0.0, math.nan, 0.25]), "t_leave": np.array([1.0, math.nan, 0.5]),
            "length": rng.random(3), "covered_length": rng.random(3), "t0": t0, "t1": t0 + 0.125,
            "level": np.array([0, 1, -1, 2, 2, 1, 0], dtype=np.int8), "fields": fields,
            "integrals": {name: rng.standard_normal(3) for name in fields}}


def test_an_npz_file_round_trips(tmp_path):
    result = _result()
    path = str(tmp_path / "rays.npz")
    ray_rules.save_npz(result, path)
    back = ray_rules.load_npz(path)
    assert back["n"] == 3 and isinstance(back["n"], int)
    assert set(back) == set(result) and list(back["fields"]) == list(result["fields"])
    for key, value in result.items():
        if key in ("fields", "integrals"):
            for name in value:
                assert ref.same_bits(back[key][name], value[name])
        elif key != "n":
            assert back[key].dtype == value.dtype and back[key].tobytes() == value.tobytes()
    empty = {**result, "n": 0, "fields": {}, "integrals": {}}
    ray_rules.save_npz(empty, path)
    assert ray_rules.load_npz(path)["fields"] == {}


def test_segment_midpoints_and_end_points():
    result = _result()
    middle = ray_rules.segment_midpoints(result)
    assert middle.shape == (7, 3)
    t = 0.5 * (result["t0"][4] + result["t1"][4])
    assert middle[4].tolist() == (result["start"][2] + t * (result["end"][2] - result["start"][2])).tolist()
    a, b = ray_rules.end_points([0.0, 1.0, 2.0], (3.0, 4.0, 5.0))
    assert a.shape == (1, 3) and b.tolist() == [[3.0, 4.0, 5.0]]
    assert ray_rules.end_points(np.zeros((0, 3)), np.zeros((0, 3)))[0].shape == (0, 3)
    for wrong in (([0.0, 1.0], [0.0, 1.0]), (np.zeros((2, 3)), np.zeros((3, 3))),
                  (np.zeros((2, 2)), np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            ray_rules.end_points(*wrong)


def test_the_default_max_trips_is_twice_the_finest_planes_across_the_bounding_box(three):
    # the scene's boxes as index ranges: level, first cell, cells
    boxes = [(l, lo, tuple(h - v + 1 for v, h in zip(lo, hi)))
             for l, grids in enumerate(THREE_BOXES) for lo, hi in grids]
    bounds = ray_rules.level0_bounds([b[1] for b in boxes], [b[2] for b in boxes],
                                     [b[0] for b in boxes], [2, 2])
    assert bounds == ((0, 0, 0), (11, 5, 7))
    assert ray_rules.default_max_trips(bounds, [2, 2], 3) == 8 + 2 * (12 + 6 + 8) * 4 == 216
    assert three.hierarchy().default_max_trips() == 216
    assert ray_rules.default_max_trips(bounds, [2, 2], 1) == 8 + 2 * 26
    # negative indices floor; a box without cells does not count; no cells at all
    assert ray_rules.level0_bounds([(-3, 5, -8), (100, 100, 100)], [(2, 2, 2), (0, 4, 4)], [1, 0],
                                   [4]) == ((-1, 1, -2), (-1, 1, -2))
    assert ray_rules.level0_bounds([(0, 0, 0)], [(0, 1, 1)], [0], []) is None
    assert ray_rules.default_max_trips(None, [], 1) == 8
    assert ray_rules.default_max_trips(((0, 0, 0), (2 ** 20, 0, 0)), [4] * 8, 9) == 2 ** 30


# ---- the API without a device ----------------------------------------------------------------------

def test_the_entry_is_declared_and_the_abi_version_stays(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    assert "int avr_scene_rays(avr_context *ctx, const avr_scene *field" in header
    assert len(_capi.SIGNATURES["avr_scene_rays"][1]) == 22
    assert getattr(avr_lib, "avr_scene_rays") is not None
    assert avr_lib.avr_abi_version() == 2


def _tiny_plotfile(path):
    levels = ref.make_levels([((0, 0, 0), (3, 3, 3)), ((0, 0, 0), (7, 7, 7))],
                             [[((0, 0, 0), (3, 3, 3))], [((2, 2, 2), (5, 5, 5))]], [2], 53)
    plotfile.write_plotfile(str(path), list(ref.VARIABLES), levels, (0.0, 0.0, 0.0),
                            (1.0, 1.0, 1.0), [2])
    return str(path)


def _patched(monkeypatch, differ=False):
    """api.rays without a device: _load_fields and ray_scene answer with two segments per ray
    whose start is finite; the values are the field's number of letters."""
    asked = []
    scene = lambda what: types.SimpleNamespace(local_boxes=what, scalar_transform=None)

    def fake_load_fields(plotfile_path, variables, min_level, max_level):
        asked.append(("load", tuple(variables), min_level, max_level))
        return "ctx", 0, 1, None, [scene(name) for name in variables], [0.015625, 0.001953125]

    def fake_scene(ctx, field, start, end, cell_sizes, prob_lo, ref_ratio, max_trips=None, rank=0,
                   n_ranks=1):
        assert ctx == "ctx" and len(cell_sizes) == 2 and list(ref_ratio) == [2]
        assert list(prob_lo) == [0.0, 0.0, 0.0] and start.shape == end.shape
        asked.append((field.local_boxes, max_trips, start.shape[0]))
        ok = np.isfinite(start[:, 0])
        counts = np.where(ok, 2, 0)
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        total = int(offsets[-1])
        t0 = np.tile([0.0, 0.5], total // 2)
        if differ and field.local_boxes != "u":
            t0 = t0 + 2.0 ** -40
        return {"offsets": offsets, "status": np.where(ok, 0, 3).astype(np.uint8),
                "t_enter": np.where(ok, 0.0, math.nan), "t_leave": np.where(ok, 1.0, math.nan),
                "integral": np.where(ok, float(len(field.local_boxes)), 0.0),
                "covered": np.where(ok, 1.0, 0.0), "t0": t0, "t1": t0 + 0.5,
                "level": np.tile(np.array([0, 1], dtype=np.int8), total // 2),
                "value": np.full(total, float(len(field.local_boxes)))}

    monkeypatch.setattr(api, "_load_fields", fake_load_fields)
    monkeypatch.setattr(api, "ray_scene", fake_scene)
    return asked


def test_api_rays_takes_the_geometry_once_and_a_value_per_field(tmp_path, monkeypatch):
    path = _tiny_plotfile(tmp_path / "plt")
    asked = _patched(monkeypatch)
    start = [[0.0, 0.5, 0.5], [math.nan, 0.5, 0.5], [0.5, 0.5, 0.0]]
    end = [[3.0, 4.5, 0.5], [1.0, 0.5, 0.5], [0.5, 0.5, 1.0]]
    out = str(tmp_path / "rays.npz")
    got = api.rays(path, start, end, fields=["whole", "u"], min_level=1, max_trips=77, output=out)
    assert asked == [("load", ("whole", "u"), 1, -1), ("whole", 77, 3), ("u", 77, 3)]
    assert got["n"] == 3 and got["offsets"].tolist() == [0, 2, 2, 4]
    assert got["status"].tolist() == [0, 3, 0] and got["length"].tolist()[::2] == [5.0, 1.0]
    assert math.isnan(got["length"][1]) and got["covered_length"].tolist() == [1.0, 0.0, 1.0]
    assert list(got["fields"]) == ["whole", "u"] and got["fields"]["u"].tolist() == [1.0] * 4
    assert got["integrals"]["whole"].tolist() == [5.0, 0.0, 5.0]
    assert got["t0"].tolist() == [0.0, 0.5, 0.0, 0.5] and got["level"].dtype == np.int8
    assert set(got) == {"n", "start", "end", "offsets", "status", "t_enter", "t_leave", "length",
                        "covered_length", "t0", "t1", "level", "fields", "integrals"}
    back = ray_rules.load_npz(out)
    assert back["n"] == 3 and ref.same_bits(back["fields"]["whole"], got["fields"]["whole"])
    assert ref.same_bits(back["integrals"]["u"], got["integrals"]["u"])
    assert ray_rules.segment_midpoints(back).tolist()[0] == [0.75, 1.5, 0.5]
    # the first variable by default; one ray as two points
    one = api.rays(path, start[0], end[0])
    assert asked[-2:] == [("load", ("u",), 0, -1), ("u", None, 1)]
    assert one["n"] == 1 and list(one["fields"]) == ["u"] and one["start"].shape == (1, 3)
    with pytest.raises(ValueError):
        api.rays(path, start, end[:2])
    with pytest.raises(RuntimeError):
        api.rays(str(tmp_path / "missing"), start, end)


def test_no_rays_give_empty_arrays(tmp_path, monkeypatch):
    path = _tiny_plotfile(tmp_path / "plt")
    _patched(monkeypatch)
    got = api.rays(path, np.zeros((0, 3)), np.zeros((0, 3)), fields=["u"],
                   output=str(tmp_path / "none.npz"))
    assert got["n"] == 0 and got["offsets"].tolist() == [0] and got["t0"].shape == (0,)
    assert got["length"].shape == (0,) and got["fields"]["u"].shape == (0,)
    assert ray_rules.load_npz(str(tmp_path / "none.npz"))["n"] == 0


def test_fields_walked_through_other_cells_are_an_error(tmp_path, monkeypatch):
    path = _tiny_plotfile(tmp_path / "plt")
    _patched(monkeypatch, differ=True)
    with pytest.raises(RuntimeError, match="t0 differs"):
        api.rays(path, [0.0, 0.5, 0.5], [1.0, 0.5, 0.5], fields=["u", "whole"])


class _HostScene:
    """A scene whose count pass finds nothing, on the CPU."""

    def __init__(self, log):
        self.log = log

    def rays(self, start, end, max_trips, index, ratios, sizes, origin, offsets=None,
             n_segments=0):
        assert offsets is None
        self.log.append((max_trips, np.asarray(index).tolist(), list(ratios), int(start.shape[0])))
        n = start.shape[0]
        return (torch.zeros(n, dtype=torch.int32), torch.full((n,), 1, dtype=torch.uint8),
                torch.full((n, 2), math.nan, dtype=torch.float64))

    def close(self):
        self.log.append("closed")


class _HostContext:
    device = torch.device("cpu")

    def __init__(self):
        self.log = []

    def create_scene(self, boxes, transform):
        return _HostScene(self.log)

    def synchronize(self):
        pass


def test_ray_scene_refuses_boxes_on_other_ranks_and_sets_the_default_max_trips():
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"the context was used ({name})")

    coarse = AmrBox((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), level=0, dims=(4, 4, 4))
    fine = AmrBox((0.25, 0.25, 0.5), (0.75, 0.5, 1.0), level=1, dims=(4, 2, 4))
    bounds = VolumeBounds((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    whole = api.SceneGeometry([coarse, fine], [coarse, fine], ScalarTransform(), bounds)
    part = api.SceneGeometry([coarse, fine], [coarse], ScalarTransform(), bounds)
    ends = ([[0.1, 0.5, 0.5]], [[0.9, 0.5, 0.6]])
    arguments = ([(0.25, 0.25, 0.25), (0.125, 0.125, 0.125)], (0.0, 0.0, 0.0), [2])
    with pytest.raises(NotImplementedError):
        api.ray_scene(NoDevice(), whole, *ends, *arguments, rank=0, n_ranks=2)
    with pytest.raises(NotImplementedError):
        api.ray_scene(NoDevice(), part, *ends, *arguments)
    ctx = _HostContext()
    got = api.ray_scene(ctx, whole, *ends, *arguments)
    # [Blo, Bhi] = [0, 3]^3, two levels of ratio 2: 8 + 2 * 12 * 2
    assert ctx.log == [(56, [[0, 0, 0], [2, 2, 4]], [2], 1), "closed"]
    assert got["offsets"].tolist() == [0, 0] and got["status"].tolist() == [1]
    assert got["t0"].shape == (0,) and got["level"].dtype == np.int8
    assert got["integral"].tolist() == [0.0] and math.isnan(got["t_enter"][0])
    ctx = _HostContext()
    api.ray_scene(ctx, whole, np.zeros((0, 3)), np.zeros((0, 3)), *arguments, max_trips=5)
    assert ctx.log[0][0] == 5 and ctx.log[0][3] == 0
    for wrong in (0, 2 ** 30 + 1):
        with pytest.raises(ValueError):
            api.ray_scene(_HostContext(), whole, *ends, *arguments, max_trips=wrong)
    with pytest.raises(ValueError):
        api.ray_scene(_HostContext(), whole, [[0.1, 0.5]], [[0.9, 0.5]], *arguments)
