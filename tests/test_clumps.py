"""Clumps, what needs no GPU: the reference against an independent construction on a uniform grid,
the registry and its refusals (cycles through all three registries), api.clumps and the loader's
name resolution with the device work patched out, and the paths that refuse before any device
work."""
import math
import os
import types

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, clumps, plotfile
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds

import clump_reference as cr
import gradient_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = math.inf


@pytest.fixture(autouse=True)
def _empty_registries():
    def clear():
        for name in list(api.clump_fields()):
            api.remove_clump_field(name)
        for name in list(api.gradient_fields()):
            api.remove_gradient_field(name)
        for name in list(api.derived_fields()):
            api.remove_field(name)
    clear()
    yield
    clear()


def test_the_entries_are_declared_and_the_abi_version_stays(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    assert "int avr_scene_clumps(avr_context *ctx, const avr_scene *in, avr_scene *out" in header
    assert "int avr_scene_clump_table(avr_context *ctx, const avr_scene *labels" in header
    assert len(_capi.SIGNATURES["avr_scene_clumps"][1]) == 9
    assert len(_capi.SIGNATURES["avr_scene_clump_table"][1]) == 8
    assert getattr(avr_lib, "avr_scene_clumps") is not None
    assert getattr(avr_lib, "avr_scene_clump_table") is not None
    assert avr_lib.avr_abi_version() == 2


# ---- the reference ---------------------------------------------------------------------------------

TWO_DOMAINS = [((0, 0, 0), (3, 3, 3)), ((0, 0, 0), (7, 7, 7))]
TWO_BOXES = [[((0, 0, 0), (3, 3, 3))], [((2, 2, 2), (5, 5, 5))]]
THREE_DOMAINS = [((0, 0, 0), (11, 5, 7)), ((0, 0, 0), (23, 11, 15)), ((0, 0, 0), (47, 23, 31))]
THREE_BOXES = [[((0, 0, 0), (6, 5, 7)), ((7, 0, 0), (11, 5, 7))],
               [((4, 2, 2), (11, 7, 9)), ((12, 2, 2), (17, 9, 9))],
               [((12, 6, 6), (21, 13, 15))]]
SKIPPED_DOMAINS = [((0, 0, 0), (7, 3, 3)), ((0, 0, 0), (15, 7, 7)), ((0, 0, 0), (31, 15, 15))]
SKIPPED_BOXES = [[((0, 0, 0), (7, 3, 3))], [((4, 2, 2), (11, 5, 5))], [((8, 4, 4), (15, 11, 11))]]


def scene_boxes(levels, ratio, min_level=0, max_level=-1):
    if max_level < 0:
        max_level = len(levels) - 1
    convex = plotfile.convexify([lev["boxes"] for lev in levels[:max_level + 1]], ratio[:max_level])
    return [(l, lo, hi) for l in range(min_level, max_level + 1) for _, (lo, hi) in convex[l]]


def uniform_labels(arrays, selected, ratio, finest):
    """Every leaf refined to level `finest` (np.repeat), holes unselected; the uniform grid
    labelled by repeated 6-neighbour minimum propagation.  Returns per level the label of each
    cell's image (that of its first fine cell), -1 where the cell is not a selected leaf."""
    shape = arrays[finest][1].shape
    chosen = np.zeros(shape, dtype=bool)
    factors = []
    for l in range(finest + 1):
        f = int(np.prod(ratio[l:finest], dtype=np.int64)) if l < finest else 1
        factors.append(f)
        image = selected[l]
        for axis in range(3):
            image = np.repeat(image, f, axis=axis)
        assert image.shape == shape
        chosen |= image
    big = np.iinfo(np.int64).max
    labels = np.where(chosen, np.arange(chosen.size, dtype=np.int64).reshape(shape), big)
    while True:
        lowest = labels.copy()
        for axis in range(3):
            for shift in (1, -1):
                moved = np.full(shape, big, dtype=np.int64)
                src = [slice(None)] * 3
                dst = [slice(None)] * 3
                src[axis] = slice(0, -1) if shift == 1 else slice(1, None)
                dst[axis] = slice(1, None) if shift == 1 else slice(0, -1)
                moved[tuple(dst)] = labels[tuple(src)]
                lowest = np.minimum(lowest, moved)
        lowest = np.where(chosen, lowest, big)
        if np.array_equal(lowest, labels):
            break
        labels = lowest
    return [np.where(selected[l], labels[::f, ::f, ::f], -1) for l, f in enumerate(factors)]


@pytest.mark.parametrize("domains, boxes, ratio, levels_loaded", [
    (TWO_DOMAINS, TWO_BOXES, [2], (0, -1)), (TWO_DOMAINS, TWO_BOXES, [2], (1, -1)),
    (TWO_DOMAINS, TWO_BOXES, [2], (0, 0)), (THREE_DOMAINS, THREE_BOXES, [2, 2], (0, -1)),
    (THREE_DOMAINS, THREE_BOXES, [2, 2], (1, -1)), (SKIPPED_DOMAINS, SKIPPED_BOXES, [2, 2], (0, -1)),
    ([((0, 0, 0), (5, 3, 3)), ((0, 0, 0), (23, 15, 15))],
     [[((0, 0, 0), (5, 3, 3))], [((8, 4, 4), (15, 11, 11))]], [4], (0, -1)),
])
def test_the_reference_equals_labelling_a_uniform_grid(domains, boxes, ratio, levels_loaded):
    levels = ref.make_levels(domains, boxes, ratio, 21)
    lo, hi = levels_loaded
    order = scene_boxes(levels, ratio, lo, hi)
    for component, bounds in ((0, (-0.5, INF)), (0, (0.4, INF)), (1, (-INF, 0.3)), (2, (-300.0, 300.0)),
                              (0, (-INF, INF)), (0, (50.0, 60.0))):
        dense, n = cr.clump_levels(levels, ratio, component, *bounds, order, lo, hi)
        arrays, finest = ref.leaf_arrays(levels, ratio, component, lo, hi)
        selected = cr.selected_arrays(arrays, *bounds)
        images = uniform_labels(arrays, selected, ratio, finest)
        ordinals, _ = cr.ordinal_arrays(levels, order)
        forward, backward, smallest = {}, {}, {}
        for l in range(finest + 1):
            assert np.array_equal(dense[l] > 0.0, selected[l])
            for label, image, ordinal in zip(dense[l][selected[l]].tolist(),
                                             images[l][selected[l]].tolist(),
                                             ordinals[l][selected[l]].tolist()):
                assert forward.setdefault(label, image) == image      # one clump, one component
                assert backward.setdefault(image, label) == label     # one component, one clump
                smallest[label] = min(smallest.get(label, ordinal), ordinal)
        assert sorted(forward) == [float(c) for c in range(1, n + 1)]
        firsts = [smallest[float(c)] for c in range(1, n + 1)]
        assert firsts == sorted(firsts) and len(set(firsts)) == n     # numbered by smallest ordinal
        if bounds == (50.0, 60.0):
            assert n == 0


def test_the_reference_table_follows_the_order_of_the_rules():
    labels = [np.array([[[0.0, 1.0, 2.0, 2.0, 1.5, 3.0, -0.0, np.nan, 2.0]]])]
    values = [np.array([[[np.nan, 1.0, 2.0, np.inf, np.nan, np.nan, 1.0, 1.0, 0.5]]])]
    mask = [np.ones((1, 1, 9), dtype=bool)]
    cells, sums, abs_sums, outside, nonfinite = cr.clump_table(labels, 2, mask, values)
    assert cells.tolist() == [[1, 2]] and sums.tolist() == [[1.0, 2.5]]
    assert (outside, nonfinite) == (4, 1)                 # 1.5, 3.0, -0.0, NaN; the +Inf under 2
    cells, sums, _, outside, nonfinite = cr.clump_table(labels, 2, mask)
    assert cells.tolist() == [[1, 3]] and sums is None and (outside, nonfinite) == (4, 0)


# ---- the registry ----------------------------------------------------------------------------------

def test_the_registry_registers_lists_and_removes():
    api.add_clump_field("cores", "density", 100.0)
    api.add_clump_field("band", "density", -1.0, 1.0)
    api.add_clump_field("all", "density")
    api.add_gradient_field("drho_dx", "density", "x")
    api.add_clump_field("steep", "drho_dx", 3.0)                # of a gradient field
    api.add_field("speed", "sqrt(u ** 2)")
    api.add_clump_field("fast", "speed", 2.0, INF)              # of a derived field
    api.add_clump_field("nested", "cores", 1.0, 1.0)            # of another clump field
    assert api.clump_fields() == {"cores": ("density", 100.0, INF), "band": ("density", -1.0, 1.0),
                                  "all": ("density", -INF, INF), "steep": ("drho_dx", 3.0, INF),
                                  "fast": ("speed", 2.0, INF), "nested": ("cores", 1.0, 1.0)}
    program = api.add_field("core_mass", "where(cores == 3, density, 0)")
    assert program.fields == ("cores", "density")               # a clump name stays a field
    api.remove_clump_field("band")
    assert "band" not in api.clump_fields()
    with pytest.raises(KeyError):
        api.remove_clump_field("band")


def test_the_registry_refuses_names_bounds_and_cycles_through_three_registries():
    for bad in ("", "x", "dz", "level", "sqrt", "where", "field", "cell_volume", "cells", None, 3):
        with pytest.raises(ValueError):
            api.add_clump_field(bad, "u")
    with pytest.raises(ValueError):
        api.add_clump_field("c", "")
    for lower, upper in ((math.nan, 1.0), (0.0, math.nan), (1.0, 0.5), (INF, -INF)):
        with pytest.raises(ValueError):
            api.add_clump_field("c", "u", lower, upper)
    api.add_field("speed", "sqrt(u ** 2)")
    api.add_gradient_field("g", "u", 0)
    with pytest.raises(ValueError, match="registered derived field"):
        api.add_clump_field("speed", "u")
    with pytest.raises(ValueError, match="registered gradient field"):
        api.add_clump_field("g", "u")
    api.add_clump_field("c", "u", 0.0)
    with pytest.raises(ValueError, match="registered clump field"):
        api.add_field("c", "u + 1")
    with pytest.raises(ValueError, match="registered clump field"):
        api.add_gradient_field("c", "u", 0)
    # cycles: of itself, through another clump field, and through all three registries, closed from
    # each registry's side
    with pytest.raises(ValueError, match="cycle"):
        api.add_clump_field("self", "self")
    api.add_clump_field("a", "b")
    with pytest.raises(ValueError, match="cycle"):
        api.add_clump_field("b", "a")
    api.add_gradient_field("da", "a", 0)
    api.add_field("twice", "2 * field('da')")
    with pytest.raises(ValueError, match="cycle"):
        api.add_clump_field("b", "twice")                       # b -> twice -> da -> a -> b
    api.add_clump_field("k", "dk")
    api.add_field("dk2", "k + 1")
    with pytest.raises(ValueError, match="cycle"):
        api.add_gradient_field("dk", "dk2", 1)                  # dk -> dk2 -> k -> dk
    api.add_clump_field("m", "later")
    api.add_gradient_field("dm", "m", 2)
    with pytest.raises(ValueError, match="cycle"):
        api.add_field("later", "dm * 2")                        # later -> dm -> m -> later
    assert "b" not in api.clump_fields() and "self" not in api.clump_fields()
    assert "dk" not in api.gradient_fields() and "later" not in api.derived_fields()


# ---- the loader and api.clumps ---------------------------------------------------------------------

def _tiny_plotfile(path):
    levels = ref.make_levels(TWO_DOMAINS, TWO_BOXES, [2], 5)
    plotfile.write_plotfile(str(path), list(ref.VARIABLES), levels, (0.0, 0.0, 0.0),
                            (1.0, 1.0, 1.0), [2])
    return str(path)


def test_the_loader_resolves_clump_names_once_per_call_and_flags(tmp_path, monkeypatch):
    path = _tiny_plotfile(tmp_path / "plt")
    calls = []

    def fake_scene(what):
        return types.SimpleNamespace(all_boxes=[types.SimpleNamespace(level=1)], local_boxes=[],
                                     what=what)

    def fake_load(ctx, plotfile_path, name, min_level, max_level, log, normalize, *rest):
        calls.append(("load", name, log, normalize))
        return fake_scene(name)

    def fake_clumps(ctx, scene, lower, upper, cell_sizes, prob_lo, ref_ratio, rank, n_ranks, group,
                    log, normalize):
        calls.append(("clumps", scene.what, lower, upper, log, normalize))
        assert len(cell_sizes) == 2 and list(ref_ratio) == [2] and tuple(prob_lo) == (0.0, 0.0, 0.0)
        return fake_scene(f"clumps({scene.what})"), 3

    def fake_gradient(ctx, scene, axis, cell_sizes, prob_lo, ref_ratio, rank, n_ranks, group, log,
                      normalize):
        calls.append(("gradient", scene.what, axis, log, normalize))
        return fake_scene(f"d({scene.what})/d{axis}")

    def fake_derive(ctx, program, scenes, geometry, cell_sizes, rank, n_ranks, group, log,
                    normalize):
        calls.append(("derive", tuple(s.what for s in scenes), log, normalize))
        return fake_scene("(" + ",".join(s.what for s in scenes) + ")")

    monkeypatch.setattr(plotfile, "load_plotfile_geometry", fake_load)
    monkeypatch.setattr(api, "clump_scene", fake_clumps)
    monkeypatch.setattr(api, "gradient_scene", fake_gradient)
    monkeypatch.setattr(api, "derive_scene", fake_derive)
    api.add_clump_field("cores", "u", 0.5)
    api.add_gradient_field("du_dx", "u", "x")
    api.add_clump_field("steep", "du_dx", -1.0, 1.0)
    api.add_field("core_u", "where(cores == 2, u, 0)")
    scenes = api._load_variable_scenes(None, path, ["core_u", "cores", "steep"], 0, -1, True, False,
                                       0, 1, None)
    assert [s.what for s in scenes] == ["(clumps(u),u)", "clumps(u)", "clumps(d(u)/d0)"]
    # inner scenes are raw (False, True) and made once; the caller's flags reach the outermost only
    assert calls == [
        ("load", "u", False, True), ("clumps", "u", 0.5, INF, False, True),
        ("derive", ("clumps(u)", "u"), True, False),
        ("clumps", "u", 0.5, INF, True, False),
        ("gradient", "u", 0, False, True), ("clumps", "d(u)/d0", -1.0, 1.0, True, False),
    ]
    api.add_clump_field("lost", "nothing")
    with pytest.raises(RuntimeError, match="'nothing' .needed by clump field 'lost'. not found"):
        api._load_variable_scenes(None, path, ["lost"], 0, -1, False, True, 0, 1, None)


class FakeContext:
    """A context whose scenes answer clump_table from prepared arrays, on the host."""

    def __init__(self, tables):
        self.tables = tables
        self.asked = []

    def synchronize(self):
        pass

    def create_scene(self, boxes, transform):
        ctx = self

        class Scene:
            def __init__(self, what):
                self.what = what

            def clump_table(self, n, n_levels, field=None):
                ctx.asked.append((self.what, n, n_levels, None if field is None else field.what))
                cells, sums, totals = ctx.tables[None if field is None else field.what]
                return (torch.from_numpy(cells), None if field is None else torch.from_numpy(sums),
                        torch.tensor(totals, dtype=torch.int64))

            def close(self):
                pass
        return Scene(boxes)


def _patched_clumps(monkeypatch, path, n, tables):
    ctx = FakeContext(tables)
    scene = lambda what: types.SimpleNamespace(local_boxes=what, scalar_transform=None)

    def fake_load_fields(plotfile_path, variables, min_level, max_level):
        return ctx, 0, 1, None, [scene(name) for name in variables], [0.5, 0.0625]

    def fake_clumps(ctx_, inner, lower, upper, cell_sizes, prob_lo, ref_ratio, rank, world, group):
        assert inner.local_boxes == "u" and (lower, upper) == (0.25, INF)
        assert len(cell_sizes) == 2 and list(ref_ratio) == [2]
        return scene("labels"), n

    monkeypatch.setattr(api, "_load_fields", fake_load_fields)
    monkeypatch.setattr(api, "clump_scene", fake_clumps)
    return ctx


def test_api_clumps_assembles_the_table(tmp_path, monkeypatch):
    path = _tiny_plotfile(tmp_path / "plt")
    cells = np.array([[3, 0, 5], [8, 1, 0]], dtype=np.int64)
    sums = np.array([[1.5, 0.0, -2.0], [0.25, 3.0, 0.0]])
    ctx = _patched_clumps(monkeypatch, path, 3, {None: (cells, None, [2, 0]),
                                                 "odd": (cells, sums, [2, 4]),
                                                 "whole": (cells, 2.0 * sums, [2, 1])})
    got = api.clumps(path, "u", 0.25, fields=["odd", "whole"])
    assert ctx.asked == [("labels", 3, 2, None), ("labels", 3, 2, "odd"), ("labels", 3, 2, "whole")]
    assert got["n"] == 3 and got["outside"] == 2 and got["nonfinite"] == 5
    assert np.array_equal(got["cells_by_level"], cells) and got["cells"].tolist() == [11, 1, 5]
    assert got["cells_by_level"].dtype == np.int64
    assert got["volume"].tolist() == [0.0 + 0.5 * 3.0 + 0.0625 * 8.0, 0.0625, 2.5]
    assert got["integrals"]["odd"].tolist() == [0.75 + 0.0625 * 0.25, 0.1875, -1.0]
    assert got["integrals"]["whole"].tolist() == [2 * (0.75 + 0.0625 * 0.25), 0.375, -2.0]
    with pytest.raises(ValueError):
        api.clumps(path, "u", math.nan)
    with pytest.raises(ValueError):
        api.clumps(path, "u", 1.0, 0.0)


def test_no_clumps_give_empty_arrays_without_a_table_call(tmp_path, monkeypatch):
    path = _tiny_plotfile(tmp_path / "plt")
    ctx = _patched_clumps(monkeypatch, path, 0, {})
    got = api.clumps(path, "u", 0.25, fields=["odd"])
    assert ctx.asked == []
    assert got["n"] == 0 and got["outside"] == 0 and got["nonfinite"] == 0
    assert got["cells_by_level"].shape == (2, 0) and got["cells_by_level"].dtype == np.int64
    assert got["cells"].shape == (0,) and got["volume"].shape == (0,)
    assert got["integrals"]["odd"].shape == (0,) and got["integrals"]["odd"].dtype == np.float64


def test_boxes_on_other_ranks_are_refused_before_any_device_work():
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"the context was used ({name})")

    box = AmrBox((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), level=0, dims=(4, 4, 4))
    bounds = VolumeBounds((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    whole = api.SceneGeometry([box, box], [box, box], ScalarTransform(), bounds)
    part = api.SceneGeometry([box, box], [box], ScalarTransform(), bounds)
    arguments = ([(0.25, 0.25, 0.25)], (0.0, 0.0, 0.0), [])
    with pytest.raises(NotImplementedError):
        api.clump_scene(NoDevice(), whole, 0.0, 1.0, *arguments, rank=0, n_ranks=2)
    with pytest.raises(NotImplementedError):
        api.clump_scene(NoDevice(), part, 0.0, 1.0, *arguments)
    with pytest.raises(ValueError, match="NaN"):
        api.clump_scene(NoDevice(), whole, math.nan, 1.0, *arguments)
    with pytest.raises(ValueError, match="exceed"):
        api.clump_scene(NoDevice(), whole, 2.0, 1.0, *arguments)


def test_volumes_and_integrals_add_the_levels_in_ascending_order():
    cells = np.array([[1, 2], [3, 4], [5, 6]], dtype=np.int64)
    volumes = [0.1, 0.01, 0.001]
    want = (0.0 + np.float64(0.1) * 1.0) + np.float64(0.01) * 3.0
    want = want + np.float64(0.001) * 5.0
    assert clumps.clump_volumes(cells, volumes)[0] == want
    assert clumps.clump_volumes(np.zeros((3, 0), dtype=np.int64), volumes).shape == (0,)
    sums = np.array([[1.0], [10.0], [100.0]])
    assert clumps.clump_integrals(sums, volumes)[0] == (0.0 + 0.1 * 1.0 + 0.01 * 10.0) + 0.001 * 100.0
