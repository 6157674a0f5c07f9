"""Gradient fields, what needs no GPU: the reference against a cell-by-cell restatement, the
registry and its refusals, the recovery of box indices, the loader's name resolution (with the
device work patched out) and the paths that refuse before any device work."""
import os
import types

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, derive, gradient, plotfile
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds

import gradient_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _empty_registries():
    def clear():
        for name in list(api.gradient_fields()):
            api.remove_gradient_field(name)
        for name in list(api.derived_fields()):
            api.remove_field(name)
    clear()
    yield
    clear()


def test_the_entry_is_declared_and_the_abi_version_stays(avr_lib):
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    assert "int avr_scene_gradient(avr_context *ctx, const avr_scene *in, avr_scene *out" in header
    assert len(_capi.SIGNATURES["avr_scene_gradient"][1]) == 8
    assert getattr(avr_lib, "avr_scene_gradient") is not None
    assert avr_lib.avr_abi_version() == 2


# ---- the reference ---------------------------------------------------------------------------------

TWO_DOMAINS = [((0, 0, 0), (3, 3, 3)), ((0, 0, 0), (7, 7, 7))]
TWO_BOXES = [[((0, 0, 0), (3, 3, 3))], [((2, 2, 2), (5, 5, 5))]]


@pytest.mark.parametrize("levels_loaded", [(0, -1), (1, -1), (0, 0)])
def test_the_reference_equals_a_cell_by_cell_loop(levels_loaded):
    levels = ref.make_levels(TWO_DOMAINS, TWO_BOXES, [2], 11)
    sizes = ref.cell_sizes(levels, (0.0, 0.0, 0.0), (1.0, 2.0, 4.0))
    lo, hi = levels_loaded
    for component in (0, 1):
        for axis in range(3):
            dense, arrays = ref.gradient_levels(levels, [2], sizes, axis, component, lo, hi)
            loop = ref.brute_force(levels, [2], sizes, axis, component, lo, hi)
            leaves = sum(int(mask.sum()) for _, mask, _ in arrays)
            assert leaves == len(loop) == {(0, -1): 56 + 64, (1, -1): 64, (0, 0): 64}[levels_loaded]
            for (l, i, j, k), want in loop.items():
                assert arrays[l][1][k, j, i]
                assert ref.same_bits(dense[l][k, j, i], want), (axis, l, i, j, k)
            if hi != 0:     # with max_level = 0 the covered (poisoned) coarse cells are leaves
                assert not any(abs(v) > 1e20 for v in loop.values() if np.isfinite(v))


def test_a_linear_field_has_the_exact_slope_everywhere():
    shape = (3, 5, 8)
    ramp = 3.0 * np.arange(8, dtype=np.float64)[None, None, :] * np.ones(shape)
    levels = [{"domain": ((0, 0, 0), (7, 4, 2)), "boxes": [((0, 0, 0), (7, 4, 2))],
               "data": [ramp[None]]}]
    sizes = ref.cell_sizes(levels, (0.0, 0.0, 0.0), (2.0, 5.0, 3.0))
    assert sizes[0][0] == 0.25
    dense, _ = ref.gradient_levels(levels, [], sizes, 0, 0)
    assert ref.same_bits(dense[0], np.full(shape, 3.0 / 0.25))       # boundary cells included
    for axis in (1, 2):
        assert ref.same_bits(ref.gradient_levels(levels, [], sizes, axis, 0)[0][0], np.zeros(shape))


# ---- the registry ----------------------------------------------------------------------------------

def test_the_registry_registers_lists_and_removes():
    api.add_gradient_field("dux_dy", "u", 1)
    api.add_gradient_field("d2u", "dux_dy", "y")                # a second derivative
    api.add_field("speed", "sqrt(u ** 2 + v ** 2)")
    api.add_gradient_field("dspeed_dz", "speed", "z")           # of a derived field
    assert api.gradient_fields() == {"dux_dy": ("u", 1), "d2u": ("dux_dy", 1),
                                     "dspeed_dz": ("speed", 2)}
    program = api.add_field("vort_z", "field('dvy_dx') - field('dux_dy')")
    assert program.fields == ("dvy_dx", "dux_dy")               # gradient names stay fields
    api.remove_gradient_field("d2u")
    assert "d2u" not in api.gradient_fields()
    with pytest.raises(KeyError):
        api.remove_gradient_field("d2u")


def test_the_registry_refuses_reserved_names_foreign_names_and_cycles():
    for bad in ("", "x", "dz", "level", "sqrt", "where", "field", "cell_volume", "cells", None, 3):
        with pytest.raises(ValueError):
            api.add_gradient_field(bad, "u", 0)
    for bad_axis in (3, -1, "w", None, 1.5, True):
        with pytest.raises(ValueError):
            api.add_gradient_field("g", "u", bad_axis)
    with pytest.raises(ValueError):
        api.add_gradient_field("g", "", 0)
    api.add_field("speed", "sqrt(u ** 2)")
    with pytest.raises(ValueError, match="registered derived field"):
        api.add_gradient_field("speed", "u", 0)
    api.add_gradient_field("g", "u", 0)
    with pytest.raises(ValueError, match="registered gradient field"):
        api.add_field("g", "u + 1")
    # cycles: of itself, through another gradient, through a derived field -- from either side
    with pytest.raises(ValueError, match="cycle"):
        api.add_gradient_field("self", "self", 0)
    api.add_gradient_field("a", "b", 0)
    with pytest.raises(ValueError, match="cycle"):
        api.add_gradient_field("b", "a", 1)
    api.add_field("twice", "2 * field('a')")
    with pytest.raises(ValueError, match="cycle"):
        api.add_gradient_field("b", "twice", 1)
    api.add_gradient_field("c", "later", 0)
    with pytest.raises(ValueError, match="cycle"):
        api.add_field("later", "c + 1")
    assert "later" not in api.derived_fields() and "b" not in api.gradient_fields()
    assert "self" not in api.gradient_fields()


# ---- index recovery --------------------------------------------------------------------------------

def test_box_indices_are_recovered_from_the_corners():
    sizes = [(0.5, 0.25, 0.125), (0.25, 0.125, 0.0625)]
    prob_lo = (-1.0, 2.0, 0.0)
    scale = 0.25
    corners = [tuple((prob_lo[a] + index[a] * sizes[level][a]) * scale for a in range(3))
               for level, index in ((0, (0, 3, 5)), (1, (-4, 7, 1000000)))]
    got = gradient.box_index_lo(corners, [0, 1], scale, prob_lo, sizes)
    assert got.dtype == np.int32 and got.tolist() == [[0, 3, 5], [-4, 7, 1000000]]
    # a scale that is no power of two still lands within 1e-6
    third = [tuple((prob_lo[a] + 7 * sizes[0][a]) / 3.0 for a in range(3))]
    assert gradient.box_index_lo(third, [0], 1.0 / 3.0, prob_lo, sizes).tolist() == [[7, 7, 7]]
    shifted = [(corners[0][0] + 1e-5 * sizes[0][0] * scale,) + corners[0][1:]]
    with pytest.raises(ValueError, match="not an integer"):
        gradient.box_index_lo(shifted, [0], scale, prob_lo, sizes)
    with pytest.raises(ValueError, match="not an integer"):
        gradient.box_index_lo([(float("nan"), 0.0, 0.0)], [0], scale, prob_lo, sizes)


# ---- the loader ------------------------------------------------------------------------------------

def _tiny_plotfile(path):
    levels = ref.make_levels(TWO_DOMAINS, TWO_BOXES, [2], 5)
    plotfile.write_plotfile(str(path), list(ref.VARIABLES), levels, (0.0, 0.0, 0.0),
                            (1.0, 1.0, 1.0), [2])
    return str(path)


def test_the_loader_resolves_gradient_names_once_per_call_and_flags(tmp_path, monkeypatch):
    path = _tiny_plotfile(tmp_path / "plt")
    calls = []

    def fake_scene(what):
        return types.SimpleNamespace(all_boxes=[types.SimpleNamespace(level=1)], local_boxes=[],
                                     what=what)

    def fake_load(ctx, plotfile_path, name, min_level, max_level, log, normalize, *rest):
        calls.append(("load", name, log, normalize))
        return fake_scene(name)

    def fake_gradient(ctx, scene, axis, cell_sizes, prob_lo, ref_ratio, rank, n_ranks, group, log,
                      normalize):
        calls.append(("gradient", scene.what, axis, log, normalize))
        assert len(cell_sizes) == 2 and list(ref_ratio) == [2] and tuple(prob_lo) == (0.0, 0.0, 0.0)
        return fake_scene(f"d({scene.what})/d{axis}")

    def fake_derive(ctx, program, scenes, geometry, cell_sizes, rank, n_ranks, group, log,
                    normalize):
        calls.append(("derive", tuple(s.what for s in scenes), log, normalize))
        return fake_scene("(" + ",".join(s.what for s in scenes) + ")")

    monkeypatch.setattr(plotfile, "load_plotfile_geometry", fake_load)
    monkeypatch.setattr(api, "gradient_scene", fake_gradient)
    monkeypatch.setattr(api, "derive_scene", fake_derive)
    api.add_gradient_field("dvy_dx", "odd", "x")
    api.add_gradient_field("dux_dy", "u", "y")
    api.add_field("vort_z", "field('dvy_dx') - field('dux_dy')")
    api.add_gradient_field("d2", "dux_dy", 1)
    api.add_gradient_field("dvort", "vort_z", 2)
    scenes = api._load_variable_scenes(None, path, ["vort_z", "u", "dux_dy", "d2", "dvort"], 0, -1,
                                       True, False, 0, 1, None)
    assert [s.what for s in scenes] == ["(d(odd)/d0,d(u)/d1)", "u", "d(u)/d1", "d(d(u)/d1)/d1",
                                        "d((d(odd)/d0,d(u)/d1))/d2"]
    # inner scenes are raw (False, True) and made once; the caller's flags reach the outermost only
    assert calls == [
        ("load", "odd", False, True), ("gradient", "odd", 0, False, True),
        ("load", "u", False, True), ("gradient", "u", 1, False, True),
        ("derive", ("d(odd)/d0", "d(u)/d1"), True, False),
        ("load", "u", True, False),
        ("gradient", "u", 1, True, False),
        ("gradient", "d(u)/d1", 1, True, False),
        ("derive", ("d(odd)/d0", "d(u)/d1"), False, True),
        ("gradient", "(d(odd)/d0,d(u)/d1)", 2, True, False),
    ]
    api.add_gradient_field("lost", "nothing", 0)
    with pytest.raises(RuntimeError, match="'nothing' .needed by gradient field 'lost'. not found"):
        api._load_variable_scenes(None, path, ["lost"], 0, -1, False, True, 0, 1, None)
    api.add_field("uses_lost", "lost * 2")
    with pytest.raises(RuntimeError, match="'nothing' .needed by gradient field 'lost'. not found"):
        api._check_derived_inputs(path, plotfile.PlotFileData(path), "uses_lost",
                                  derive.compile_field("uses_lost"))
    api._check_derived_inputs(path, plotfile.PlotFileData(path), "vort_z",
                              derive.compile_field("vort_z"))


def test_boxes_on_other_ranks_are_refused_before_any_device_work():
    class NoDevice:
        def __getattr__(self, name):
            raise AssertionError(f"the context was used ({name})")

    box = AmrBox((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), level=0, dims=(4, 4, 4))
    bounds = VolumeBounds((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    whole = api.SceneGeometry([box, box], [box, box], ScalarTransform(), bounds)
    part = api.SceneGeometry([box, box], [box], ScalarTransform(), bounds)
    arguments = (0, [(0.25, 0.25, 0.25)], (0.0, 0.0, 0.0), [])
    with pytest.raises(NotImplementedError):
        api.gradient_scene(NoDevice(), whole, *arguments, rank=0, n_ranks=2)
    with pytest.raises(NotImplementedError):
        api.gradient_scene(NoDevice(), part, *arguments)
    with pytest.raises(ValueError, match="axis"):
        api.gradient_scene(NoDevice(), whole, 3, *arguments[1:])
