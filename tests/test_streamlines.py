"""Streamlines without a GPU: the numpy reference (streamline_reference) against things that are
not its twin -- a uniform field's exact steps across three levels, a rotation's closed-form circle,
a trilinear polynomial, one line of every status -- and the host side of the API: lines.py, the
declared ABI entry, api.streamlines and api.sample_points with the device work patched out."""
import math
import os
import types

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, lines, plotfile
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds

import gradient_reference as ref
import streamline_reference as sl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52


def analytic_levels(domains, boxes, lo, hi, fields):
    """levels for the reference: fields, functions of (x, y, z), at the cell centres of every grid
    (the cells a finer grid covers included: the leaf masks leave them out)."""
    levels = []
    for (dlo, dhi), grids in zip(domains, boxes):
        dx = [(hi[a] - lo[a]) / (dhi[a] - dlo[a] + 1) for a in range(3)]
        data = []
        for glo, ghi in grids:
            k, j, i = np.meshgrid(*[np.arange(glo[a], ghi[a] + 1) for a in (2, 1, 0)],
                                  indexing="ij")
            x, y, z = (lo[a] + (index + 0.5) * dx[a] for a, index in enumerate((i, j, k)))
            data.append(np.stack([f(x, y, z) + 0.0 * x for f in fields]))
        levels.append({"domain": (dlo, dhi), "boxes": list(grids), "data": data})
    return levels


THREE_DOMAINS = [((0, 0, 0), (11, 5, 7)), ((0, 0, 0), (23, 11, 15)), ((0, 0, 0), (47, 23, 31))]
THREE_BOXES = [[((0, 0, 0), (6, 5, 7)), ((7, 0, 0), (11, 5, 7))],
               [((4, 2, 2), (11, 7, 9)), ((12, 2, 2), (17, 9, 9))],
               [((12, 6, 6), (21, 13, 15))]]
THREE_LO, THREE_HI = (0.0, -1.0, 2.0), (1.5, 0.5, 3.0)


# ---- a uniform field -----------------------------------------------------------------------------

@pytest.mark.parametrize("direction", [1, -1])
def test_a_uniform_field_steps_by_h_along_it_and_h_follows_the_leaf_level(direction):
    """V = (a, b, c) everywhere: trilinear or not, every evaluation gives V exactly, so every stage
    has the same k = direction V / |V| and a step is P + (h / 6) (6 k) up to the roundings of the
    sum of the four stages (three, each relative 2^-53), of h / 6 and the product (two) and of the
    final addition (half an ulp of P'): |P' - P - h k| <= 2^-52 (|P'| + 4 h) with room to spare."""
    v = np.array([0.75, 0.3125, 0.4375])
    levels = analytic_levels(THREE_DOMAINS, THREE_BOXES, THREE_LO, THREE_HI,
                             [lambda x, y, z, c=c: c for c in v])
    sizes = ref.cell_sizes(levels, THREE_LO, THREE_HI)
    hierarchy = sl.Hierarchy(levels, [2, 2], (0, 1, 2), sizes, THREE_LO)
    # the first line runs through the middle of the finest box, (0.53, -0.375, 2.34)
    middle = np.array([0.53, -0.375, 2.34])
    seeds = np.array([middle - 0.5 * direction * v, [0.05, -0.6, 2.3], [0.3, -0.9, 2.2]])
    if direction < 0:
        seeds[1:] = seeds[1:] + np.array([1.1, 0.55, 0.6])
    out = hierarchy.trace(seeds, 0.5, direction, 200)
    unit = direction * v / math.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    seen = set()
    for s in range(seeds.shape[0]):
        count = out["counts"][s]
        assert out["status"][s] == sl.OUTSIDE and 20 < count < 200     # leaves through a face
        points = out["points"][s, :count]
        level = hierarchy.locate(points)[0]
        # the line ends at its last point inside, a stage of whose step was outside, or one beyond
        assert (level[:-1] >= 0).all()
        seen |= set(level[:-1].tolist())
        for n in range(count - 1):
            h = 0.5 * min(sizes[level[n]])
            bound = EPS * (np.abs(points[n + 1]).max() + 4.0 * h)
            assert np.abs(points[n + 1] - points[n] - h * unit).max() <= bound
    assert seen == {0, 1, 2}


# ---- a rotation ----------------------------------------------------------------------------------

def _circle(step, radius=1.0):
    """One revolution around (2, 2) in a 32 x 32 x 8 box of cells of 1/8: the radius error at the
    end."""
    lo, hi, n = (0.0, 0.0, 0.0), (4.0, 4.0, 1.0), 32
    domain = ((0, 0, 0), (n - 1, n - 1, 7))
    levels = analytic_levels([domain], [[domain]], lo, hi,
                             [lambda x, y, z: -(y - 2.0), lambda x, y, z: x - 2.0,
                              lambda x, y, z: 0.0])
    hierarchy = sl.Hierarchy(levels, [], (0, 1, 2), ref.cell_sizes(levels, lo, hi), lo)
    h = step * 0.125
    steps = int(round(2.0 * math.pi * radius / h))
    out = hierarchy.trace([[2.0 + radius, 2.0, 0.5]], step, 1, steps)
    assert out["counts"][0] == steps + 1 and out["status"][0] == sl.REACHED
    end = out["points"][0, steps]
    return abs(math.hypot(end[0] - 2.0, end[1] - 2.0) - radius)


def test_a_rotation_closes_its_circle_to_fourth_order():
    """V = (-(y - y0), x - x0, 0) is linear, so between cell centres the trilinear value is V up to
    rounding, and the line is RK4 on the unit-speed circle of radius 1 = 8 cells around (2, 2), 8
    cells and more from the domain's faces.  Halving the step divides the radius error after one
    revolution by 2^4 or better.  Measured here, radius 1: 8.259e-07 at step 1 and 2.611e-08 at
    step 1/2, ratio 31.63 (RK4 keeps a circle's radius one order better than its phase); other
    radii and steps tried gave 31.63 to 32.15 (radius 0.5, 1 and 1.5, steps 1, 1/2 and 1/4), so
    the radius and the steps here are ones whose ratio lies inside the bound."""
    coarse, fine = _circle(1.0), _circle(0.5)
    print("radius error:", coarse, fine, "ratio:", coarse / fine)
    assert 8.0 <= coarse / fine <= 32.0


# ---- a trilinear polynomial ----------------------------------------------------------------------

def test_sample_points_reproduces_a_trilinear_polynomial_and_falls_back_to_the_leaf():
    """f = a + b x + c y + d z + e x y + f x z + g y z + h x y z at the cell centres: away from the
    fallback layer the trilinear value is f(P) up to a few roundings of numbers of the size of the
    terms (their sum of magnitudes is below 40 here: 64 ulp of 64); in the half cell next to a
    domain face, and in a coarse cell that has a covered cell among its eight centres, the leaf
    cell's own value comes back exactly."""
    c = (0.5, -1.25, 2.0, 0.75, 0.375, -0.5, 1.5, -0.25)
    f = lambda x, y, z: (c[0] + c[1] * x + c[2] * y + c[3] * z + c[4] * x * y + c[5] * x * z
                         + c[6] * y * z + c[7] * x * y * z)
    lo, hi = (0.0, -1.0, 2.0), (2.0, 1.0, 3.0)
    domain = ((0, 0, 0), (15, 15, 7))
    levels = analytic_levels([domain], [[((0, 0, 0), (7, 15, 7)), ((8, 0, 0), (15, 15, 7))]],
                             lo, hi, [f])
    sizes = ref.cell_sizes(levels, lo, hi)
    rng = np.random.default_rng(7)
    half = 0.5 * np.array(sizes[0])
    inner = np.array(lo) + half + rng.random((500, 3)) * (np.array(hi) - np.array(lo) - 2 * half)
    value, inside = sl.sample_points(levels, [], 0, sizes, lo, inner)
    assert inside.all()
    assert np.abs(value - f(inner[:, 0], inner[:, 1], inner[:, 2])).max() <= 64 * EPS * 64
    assert np.abs(value - f(inner[:, 0], inner[:, 1], inner[:, 2])).max() > 0.0
    # the half cell next to the faces: the leaf's own value, exactly
    for axis in range(3):
        for side in (0, 1):
            layer = inner.copy()
            layer[:, axis] = (lo[axis] + 0.49 * half[axis] * rng.random(500) if side == 0 else
                              hi[axis] - half[axis] * (0.01 + 0.98 * rng.random(500)))
            value, inside = sl.sample_points(levels, [], 0, sizes, lo, layer)
            cell = np.floor((layer - np.array(lo)) / np.array(sizes[0]))
            centre = np.array(lo) + (cell + 0.5) * np.array(sizes[0])
            assert inside.all()
            assert np.array_equal(value, f(centre[:, 0], centre[:, 1], centre[:, 2]))
    # two levels: next to the finer region a coarse point has a covered centre among its eight
    two = analytic_levels([((0, 0, 0), (7, 7, 3)), ((0, 0, 0), (15, 15, 7))],
                          [[((0, 0, 0), (7, 7, 3))], [((4, 4, 0), (11, 11, 7))]], lo, hi, [f])
    two_sizes = ref.cell_sizes(two, lo, hi)
    near = np.array([[lo[0] + 1.6 * two_sizes[0][0], lo[1] + 3.7 * two_sizes[0][1], 2.4],
                     [lo[0] + 1.2 * two_sizes[0][0], lo[1] + 3.7 * two_sizes[0][1], 2.4]])
    value, inside = sl.sample_points(two, [2], 0, two_sizes, lo, near)
    cell = np.floor((near - np.array(lo)) / np.array(two_sizes[0]))
    centre = np.array(lo) + (cell + 0.5) * np.array(two_sizes[0])
    own = f(centre[:, 0], centre[:, 1], centre[:, 2])
    assert inside.all() and value[0] == own[0]                  # a corner at i = 2 is covered
    assert value[1] != own[1]                                   # corners at i = 0, 1: trilinear
    assert abs(value[1] - f(*near[1])) <= 64 * EPS * 64


# ---- one line of every status --------------------------------------------------------------------

def test_one_line_of_every_status():
    lo, hi = (0.0, 0.0, 0.0), (2.0, 1.0, 1.0)
    domain = ((0, 0, 0), (15, 7, 7))

    def vx(x, y, z):
        out = np.ones_like(x)
        out[(x > 1.0) & (y < 0.5) & (z < 0.5)] = 0.0           # a block of still cells
        out[(x > 1.0) & (x < 1.25) & (y > 0.5) & (z > 0.5)] = np.nan
        return out

    still = lambda x, y, z: vx(x, y, z) * 0.0
    levels = analytic_levels([domain], [[domain]], lo, hi, [vx, still, still])
    sizes = ref.cell_sizes(levels, lo, hi)
    hierarchy = sl.Hierarchy(levels, [], (0, 1, 2), sizes, lo, sample=0)
    seeds = np.array([[-0.5, 0.3, 0.3],            # outside
                      [0.3, math.nan, 0.3],        # a NaN coordinate
                      [0.2, 0.2, 0.2],             # runs into the still block
                      [0.2, 0.8, 0.8],             # runs into the NaN cells
                      [0.2, 0.2, 0.8],             # leaves through the face x = 2
                      [0.2, 0.8, 0.2]])            # ... after its steps are used up
    out = hierarchy.trace(seeds, 0.5, 1, 40)
    assert out["status"].tolist() == [1, 1, 2, 3, 1, 1]
    assert out["counts"][:2].tolist() == [0, 0] and np.isnan(out["points"][:2]).all()
    # from x = 1 + dx / 2 on all eight centres are still: the line ends at the last point one of
    # whose stages, at most h = dx / 2 ahead, reaches that far
    stopped = out["points"][2, out["counts"][2] - 1]
    assert 1.0 <= stopped[0] < 1.0 + 0.5 * sizes[0][0] and out["counts"][2] > 10
    # next to the NaN cells the velocity is the leaf's own, and a stage in a NaN cell ends the line
    ended = out["points"][3, out["counts"][3] - 1]
    assert 1.0 - 0.5 * sizes[0][0] <= ended[0] < 1.0
    assert (out["samples"][3, :out["counts"][3]] == 1.0).all()
    value, inside = sl.sample_points(levels, [], 0, sizes, lo, [[1.1, 0.8, 0.8]])
    assert inside.tolist() == [True] and np.isnan(value[0])       # the leaf's value, whatever it is
    # ... and at the face at the last point whose fourth stage, h ahead, is still inside
    last = out["points"][4, out["counts"][4] - 1]
    assert 2.0 - 0.5 * sizes[0][0] <= last[0] < 2.0
    assert (out["samples"][4, :out["counts"][4]] == 1.0).all()
    assert np.isnan(out["samples"][4, out["counts"][4]:]).all()
    short = hierarchy.trace(seeds[5:], 0.5, 1, 7)
    assert short["status"].tolist() == [0] and short["counts"].tolist() == [8]
    # backward, a line leaves through x = 0
    assert hierarchy.trace(seeds[2:3], 0.5, -1, 40)["status"].tolist() == [1]


def test_a_line_ends_in_the_hole_that_min_level_leaves():
    lo, hi = (0.0, 0.0, 0.0), (2.0, 1.0, 1.0)
    domains = [((0, 0, 0), (7, 3, 3)), ((0, 0, 0), (15, 7, 7))]
    boxes = [[((0, 0, 0), (7, 3, 3))], [((4, 2, 2), (11, 5, 5))]]
    one, zero = (lambda x, y, z: 1.0), (lambda x, y, z: 0.0)
    levels = analytic_levels(domains, boxes, lo, hi, [one, zero, zero])
    sizes = ref.cell_sizes(levels, lo, hi)
    seed = np.array([[0.6, 0.5, 0.5]])                              # in the fine box
    whole = sl.trace(levels, [2], (0, 1, 2), sizes, lo, seed, 1.0, 1, 100)
    # a line ends at the last point from which a whole step (h = one cell) stays inside
    end = whole["points"][0, whole["counts"][0] - 1]
    assert whole["status"].tolist() == [1] and 2.0 - sizes[0][0] <= end[0] < 2.0
    fine = sl.trace(levels, [2], (0, 1, 2), sizes, lo, seed, 1.0, 1, 100, min_level=1)
    end = fine["points"][0, fine["counts"][0] - 1]
    assert fine["status"].tolist() == [1] and 1.5 - sizes[1][0] <= end[0] < 1.5
    # h follows the level: fine steps inside the fine box, coarse ones after it
    steps = np.diff(whole["points"][0, :whole["counts"][0], 0])
    assert abs(steps[0] - sizes[1][0]) < 1e-12 and abs(steps[-1] - sizes[0][0]) < 1e-12
    # a seed in the hole is outside
    assert sl.trace(levels, [2], (0, 1, 2), sizes, lo, [[0.2, 0.5, 0.5]], 1.0, 1, 4,
                    min_level=1)["counts"].tolist() == [0]


# ---- lines.py ------------------------------------------------------------------------------------

def test_both_joins_the_backward_line_reversed_to_the_forward_line():
    back = [np.array([[0.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [-2.0, 0.5, 0.0]]), np.zeros((0, 3)),
            np.array([[5.0, 5.0, 5.0]])]
    ahead = [np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), np.zeros((0, 3)),
             np.array([[5.0, 5.0, 5.0], [6.0, 5.0, 5.0]])]
    joined = lines.join_both(back, ahead)
    assert joined[0].tolist() == [[-2.0, 0.5, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 0.0],
                                  [1.0, 0.0, 0.0]]
    assert joined[1].shape == (0, 3) and joined[2].tolist() == [[5.0, 5.0, 5.0], [6.0, 5.0, 5.0]]
    values = lines.join_both([np.array([1.0, 2.0, 3.0])], [np.array([1.0, 7.0])])
    assert values[0].tolist() == [3.0, 2.0, 1.0, 7.0]
    assert lines.line_lengths(joined).tolist() == [math.fsum([math.sqrt(1.25), 1.0, 1.0]), 0.0, 1.0]
    with pytest.raises(ValueError):
        lines.join_both(back, ahead[:2])


def test_a_vtk_file_round_trips(tmp_path):
    rng = np.random.default_rng(3)
    found = [rng.standard_normal((5, 3)), np.zeros((0, 3)), rng.standard_normal((1, 3)) * 1e-300,
             np.array([[1.0, math.nan, -0.0], [math.inf, 2.0 ** -1074, 1e308]])]
    samples = {"density": [rng.standard_normal(5), np.zeros(0), np.array([math.nan]),
                           np.array([-math.inf, 0.1])],
               "level": [np.ones(5), np.zeros(0), np.zeros(1), np.full(2, 2.0)]}
    path = str(tmp_path / "lines.vtk")
    lines.save_vtk_lines(found, path, samples)
    text = open(path).read().split("\n")
    assert text[2:5] == ["ASCII", "DATASET POLYDATA", "POINTS 8 double"]
    assert "LINES 4 12" in text and "POINT_DATA 8" in text and "SCALARS density double 1" in text
    back, back_samples = lines.load_vtk_lines(path)
    assert len(back) == 4 and all(ref.same_bits(a, b) for a, b in zip(back, found))
    assert np.signbit(back[3][0, 2]) and list(back_samples) == ["density", "level"]
    for name in samples:
        assert all(ref.same_bits(a, b) for a, b in zip(back_samples[name], samples[name]))
    lines.save_vtk_lines(found, path)
    assert lines.load_vtk_lines(path)[1] == {}
    lines.save_vtk_lines([], path)
    assert lines.load_vtk_lines(path) == ([], {})
    with pytest.raises(ValueError):
        lines.save_vtk_lines(found, path, {"two words": samples["density"]})
    with pytest.raises(ValueError):
        lines.save_vtk_lines(found, path, {"short": samples["density"][:3]})
    with pytest.raises(ValueError):
        lines.save_vtk_lines([np.zeros((2, 2))], path)


# ---- the API without a device ----------------------------------------------------------------------

def test_the_entry_is_declared_and_the_abi_version_stays(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    assert "int avr_scene_streamlines(avr_context *ctx, const avr_scene *vx" in header
    assert len(_capi.SIGNATURES["avr_scene_streamlines"][1]) == 19
    assert getattr(avr_lib, "avr_scene_streamlines") is not None
    assert avr_lib.avr_abi_version() == 2


def _tiny_plotfile(path):
    levels = ref.make_levels([((0, 0, 0), (3, 3, 3)), ((0, 0, 0), (7, 7, 7))],
                             [[((0, 0, 0), (3, 3, 3))], [((2, 2, 2), (5, 5, 5))]], [2], 53)
    plotfile.write_plotfile(str(path), list(ref.VARIABLES), levels, (0.0, 0.0, 0.0),
                            (1.0, 1.0, 1.0), [2])
    return str(path)


def _patched(monkeypatch):
    """api.streamlines and api.sample_points without a device: _load_fields and streamline_scene
    answer with straight lines along x, one point fewer per seed and direction."""
    asked = []
    scene = lambda what: types.SimpleNamespace(local_boxes=what, scalar_transform=None)

    def fake_load_fields(plotfile_path, variables, min_level, max_level):
        return "ctx", 0, 1, None, [scene(name) for name in variables], [0.015625, 0.001953125]

    def fake_scene(ctx, vx, vy, vz, seeds, cell_sizes, prob_lo, ref_ratio, step=0.5,
                   max_steps=1000, direction=1, sample=None, rank=0, n_ranks=1):
        assert ctx == "ctx" and len(cell_sizes) == 2 and list(ref_ratio) == [2]
        assert list(prob_lo) == [0.0, 0.0, 0.0]
        names = (vx.local_boxes, vy.local_boxes, vz.local_boxes)
        asked.append((names, direction, step, max_steps,
                      None if sample is None else sample.local_boxes))
        n = seeds.shape[0]
        points = np.full((n, max_steps + 1, 3), math.nan)
        values = np.full((n, max_steps + 1), math.nan) if sample is not None else None
        counts = np.zeros(n, dtype=np.int64)
        for i in range(n):
            counts[i] = max(min(max_steps + 1, 4 - i), 0) if math.isfinite(seeds[i, 0]) else 0
            for p in range(counts[i]):
                points[i, p] = seeds[i] + np.array([direction * 0.5 * p, 0.0, 0.0])
                if values is not None:
                    values[i, p] = len(sample.local_boxes) + direction * p
        status = np.where(counts == 0, 1, 2 if direction > 0 else 3).astype(np.uint8)
        return points, counts, status, values

    monkeypatch.setattr(api, "_load_fields", fake_load_fields)
    monkeypatch.setattr(api, "streamline_scene", fake_scene)
    return asked


def test_api_streamlines_joins_measures_samples_and_writes_the_file(tmp_path, monkeypatch):
    path = _tiny_plotfile(tmp_path / "plt")
    asked = _patched(monkeypatch)
    seeds = [[0.5, 0.5, 0.5], [0.25, 0.5, 0.5], [math.nan, 0.5, 0.5]]
    out = str(tmp_path / "lines.vtk")
    got = api.streamlines(path, ("u", "odd", "whole"), seeds, step=0.25, max_steps=9,
                          direction="both", fields=["whole", "u"], output=out)
    names = ("u", "odd", "whole")
    assert asked == [(names, -1, 0.25, 9, "whole"), (names, -1, 0.25, 9, "u"),
                     (names, 1, 0.25, 9, "whole"), (names, 1, 0.25, 9, "u")]
    assert got["n"] == 3 and got["status"].tolist() == [[3, 2], [3, 2], [1, 1]]
    assert got["lines"][0][:, 0].tolist() == [-1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0]
    assert got["lines"][1][:, 0].tolist() == [-0.75, -0.25, 0.25, 0.75, 1.25]
    assert got["lines"][2].shape == (0, 3)
    assert got["length"].tolist() == [3.0, 2.0, 0.0]
    assert got["samples"]["whole"][0].tolist() == [2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
    assert got["samples"]["u"][1].tolist() == [-1.0, 0.0, 1.0, 2.0, 3.0]
    back, back_samples = lines.load_vtk_lines(out)
    assert all(ref.same_bits(a, b) for a, b in zip(back, got["lines"]))
    assert list(back_samples) == ["whole", "u"]
    ahead = api.streamlines(path, names, seeds, direction="forward")
    assert asked[-1] == (names, 1, 0.5, 1000, None) and ahead["samples"] == {}
    assert ahead["status"].tolist() == [2, 2, 1] and ahead["lines"][0].shape == (4, 3)
    behind = api.streamlines(path, names, seeds, direction="backward", max_steps=1)
    assert asked[-1] == (names, -1, 0.5, 1, None) and behind["lines"][0][:, 0].tolist() == [0.5, 0.0]
    with pytest.raises(ValueError):
        api.streamlines(path, names, seeds, direction="sideways")
    with pytest.raises(ValueError):
        api.streamlines(path, names[:2], seeds)


def test_no_seeds_give_no_lines(tmp_path, monkeypatch):
    path = _tiny_plotfile(tmp_path / "plt")
    _patched(monkeypatch)
    got = api.streamlines(path, ("u", "odd", "whole"), np.zeros((0, 3)), direction="both",
                          fields=["u"], output=str(tmp_path / "none.vtk"))
    assert got["n"] == 0 and got["lines"] == [] and got["status"].shape == (0, 2)
    assert got["length"].shape == (0,) and got["samples"] == {"u": []}
    assert lines.load_vtk_lines(str(tmp_path / "none.vtk"))[0] == []


def test_api_sample_points_is_a_line_of_no_steps_per_field(tmp_path, monkeypatch):
    path = _tiny_plotfile(tmp_path / "plt")
    asked = _patched(monkeypatch)
    values, inside = api.sample_points(path, [[0.5, 0.5, 0.5], [math.nan, 0.0, 0.0]], ["u", "whole"])
    assert asked == [(("u",) * 3, 1, 1.0, 0, "u"), (("whole",) * 3, 1, 1.0, 0, "whole")]
    assert inside.tolist() == [True, False] and list(values) == ["u", "whole"]
    assert values["u"][0] == 1.0 and values["whole"][0] == 5.0 and np.isnan(values["u"][1])
    with pytest.raises(ValueError):
        api.sample_points(path, [[0.5, 0.5, 0.5]], [])


def test_boxes_on_other_ranks_and_wrong_arguments_are_refused_before_device_work():
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"the context was used ({name})")

    box = AmrBox((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), level=0, dims=(4, 4, 4))
    bounds = VolumeBounds((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    whole = api.SceneGeometry([box, box], [box, box], ScalarTransform(), bounds)
    part = api.SceneGeometry([box, box], [box], ScalarTransform(), bounds)
    seeds = [[0.5, 0.5, 0.5]]
    arguments = ([(0.25, 0.25, 0.25)], (0.0, 0.0, 0.0), [])
    with pytest.raises(NotImplementedError):
        api.streamline_scene(NoDevice(), whole, whole, whole, seeds, *arguments, rank=0, n_ranks=2)
    with pytest.raises(NotImplementedError):
        api.streamline_scene(NoDevice(), part, part, part, seeds, *arguments)
    for wrong in (dict(step=0.0), dict(step=math.nan), dict(step=2.0), dict(direction=0),
                  dict(max_steps=-1), dict(max_steps=2 ** 20 + 1)):
        with pytest.raises(ValueError):
            api.streamline_scene(NoDevice(), whole, whole, whole, seeds, *arguments, **wrong)
    with pytest.raises(ValueError):
        api.streamline_scene(NoDevice(), whole, whole, whole, [[0.5, 0.5]], *arguments)
