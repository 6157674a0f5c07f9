"""Slices, what needs no GPU: the C ABI's new entries, the unchanged ABI version, render modes and
projection quantities, the argument checks of api.slice (raised before any GPU work), the plane's
basis convention and combine_slices on hand-made parts."""
import inspect

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, runtime

NEW_SYMBOLS = ["avr_slice_scene", "avr_slice_outline"]


def test_new_symbols_resolve_in_the_library():
    handle = _capi.lib()
    for name in NEW_SYMBOLS:
        assert getattr(handle, name) is not None, name
        assert name in _capi.SIGNATURES, name


def test_abi_version_stays_two():
    assert _capi.lib().avr_abi_version() == 2


def test_render_modes_and_projection_quantities_are_unchanged():
    assert api.RENDER_MODES == ("volume", "max_intensity")
    assert runtime.PROJECTION_QUANTITIES == ("column", "mean")
    assert api.SLICE_QUANTITIES == ("value", "level")
    assert "axis" not in inspect.signature(api.render).parameters
    assert "axis" not in inspect.signature(api.project).parameters
    assert hasattr(runtime.Scene, "slice") and hasattr(runtime.Context, "slice_outline")
    defaults = {k: p.default for k, p in inspect.signature(api.slice).parameters.items()}
    assert defaults["axis"] == "z" and defaults["quantity"] == "value"
    assert defaults["width"] == defaults["height"] == 512
    assert defaults["annotate_grids"] is False and defaults["output"] is None


@pytest.mark.parametrize("kwargs,match", [
    (dict(axis="w"), "axis"),
    (dict(axis="Z"), "axis"),
    (dict(axis=2), "axis"),
    (dict(normal=(0.0, 0.0, 1.0)), "north"),
    (dict(normal=(0.0, 0.0, 1.0), north=(0.0, 0.0, 0.0)), "north"),
    (dict(normal=(0.0, 0.0, 1.0), north=(0.0, float("nan"), 1.0)), "north"),
    (dict(normal=(0.0, 0.0, 1.0), north=(0.0, 0.0, 3.0)), "parallel"),
    (dict(normal=(0.0, 0.0, 1.0), north=(0.0, 1e-7, -1.0)), "parallel"),
    (dict(normal=(0.0, 0.0, 0.0), north=(0.0, 1.0, 0.0)), "normal"),
    (dict(normal=(float("inf"), 0.0, 0.0), north=(0.0, 1.0, 0.0)), "normal"),
    (dict(normal=(1.0, 0.0), north=(0.0, 1.0, 0.0)), "normal"),
    (dict(axis="z", north=(0.0, 0.0, 1.0)), "parallel"),
    (dict(plane_width=(1.0, 0.0)), "plane_width"),
    (dict(plane_width=(-1.0, 1.0)), "plane_width"),
    (dict(plane_width=(1.0, float("inf"))), "plane_width"),
    (dict(plane_width=(float("nan"), 1.0)), "plane_width"),
    (dict(plane_width=(1.0,)), "plane_width"),
    (dict(quantity="density"), "quantity"),
    (dict(quantity="Level"), "quantity"),
    (dict(value_range=(2.0, 1.0)), "lo < hi"),
    (dict(value_range=(1.0, 1.0)), "lo < hi"),
    (dict(value_range=(0.0, float("inf"))), "finite"),
    (dict(value_range=(1.0,)), "two values"),
    (dict(value_range=(0.0, 1.0), log_scale=True), "positive"),
    (dict(width=0), "dimensions"),
    (dict(height=-3), "dimensions"),
    (dict(center=(0.0, float("nan"), 0.0)), "center"),
    (dict(center=(0.0, 1.0)), "center"),
])
def test_bad_arguments_are_refused_before_any_gpu_work(tmp_path, kwargs, match, monkeypatch):
    # no plotfile, and no runtime: the error comes first
    def no_gpu(*args, **kw):
        raise AssertionError("GPU work started")
    monkeypatch.setattr(api, "_runtime_scope", no_gpu)
    with pytest.raises(ValueError, match=match):
        api.slice(str(tmp_path / "missing"), **kwargs)


def test_good_arguments_pass_the_checks():
    normal, north, widths, rng = api.validate_slice_arguments(8, 8)
    assert (normal, north, widths, rng) == ((0.0, 0.0, 1.0), (0.0, 1.0, 0.0), None, None)
    normal, north, widths, rng = api.validate_slice_arguments(
        8, 4, "x", (1, 1, 0), (0, 0, 2), [2, 3], "level", True, (0.5, 2.0))
    assert normal == (1.0, 1.0, 0.0) and north == (0.0, 0.0, 2.0)
    assert widths == (2.0, 3.0) and rng == (0.5, 2.0)
    # north alone re-orients the axis's plane
    normal, north, _, _ = api.validate_slice_arguments(8, 8, "z", None, (1.0, 0.0, 0.0))
    assert normal == (0.0, 0.0, 1.0) and north == (1.0, 0.0, 0.0)


@pytest.mark.parametrize("axis,right,up", [("x", (0, 1, 0), (0, 0, 1)),
                                           ("y", (0, 0, 1), (1, 0, 0)),
                                           ("z", (1, 0, 0), (0, 1, 0))])
def test_axis_convention(axis, right, up):
    normal, north = api.SLICE_AXES[axis]
    n, u, v = api.slice_basis(normal, north)
    assert n == tuple(float(c) for c in normal)
    assert u == tuple(float(c) for c in right)
    assert v == tuple(float(c) for c in up)


def test_basis_of_an_oblique_plane_is_orthonormal_and_right_handed():
    n, u, v = api.slice_basis((1.0, 2.0, -0.5), (0.1, 0.2, 3.0))
    n, u, v = (np.array(e) for e in (n, u, v))
    for a in (n, u, v):
        assert abs(a @ a - 1.0) < 1e-15
    assert abs(n @ u) < 1e-15 and abs(n @ v) < 1e-15 and abs(u @ v) < 1e-15
    assert np.allclose(np.cross(u, v), n, rtol=0, atol=1e-15)   # n points at the viewer
    assert v @ np.array((0.1, 0.2, 3.0)) > 0                    # north is up


def _part(value, level, box):
    return (np.array(value, np.float64), np.array(level, np.int8), np.array(box, np.int32))


def test_combine_slices_on_hand_made_parts():
    nan, inf = float("nan"), float("inf")
    # pixels: hit by part 0 | hit by part 1 with a NaN cell | all miss | part 2 with -inf | -0.0
    a = _part([[1.5, 0.0, 0.0, 0.0, 0.0]], [[0, -1, -1, -1, -1]], [[7, -1, -1, -1, -1]])
    b = _part([[0.0, nan, 0.0, 0.0, -0.0]], [[-1, 2, -1, -1, 1]], [[-1, 0, -1, -1, 3]])
    c = _part([[0.0, 0.0, 0.0, -inf, 0.0]], [[-1, -1, -1, 1, -1]], [[-1, -1, -1, 12, -1]])
    want = _part([[1.5, nan, 0.0, -inf, -0.0]], [[0, 2, -1, 1, 1]], [[7, 0, -1, 12, 3]])
    for order in ([a, b, c], [c, a, b], [b, c, a]):
        value, level, box = api.combine_slices(order)
        assert isinstance(value, np.ndarray) and value.dtype == np.float64
        assert np.array_equal(value.view(np.uint64), want[0].view(np.uint64))
        assert level.dtype == np.int8 and np.array_equal(level, want[1])
        assert box.dtype == np.int32 and np.array_equal(box, want[2])
    # a single part comes back as it is, and the inputs are not written
    value, level, box = api.combine_slices([b])
    assert np.array_equal(value.view(np.uint64), b[0].view(np.uint64))
    assert np.array_equal(level, b[1]) and np.array_equal(box, b[2])
    assert a[0][0, 0] == 1.5 and a[1][0, 1] == -1


def test_combine_slices_takes_tensors_and_checks_its_parts():
    a = tuple(torch.from_numpy(t) for t in _part([[2.0, 0.0]], [[1, -1]], [[4, -1]]))
    b = tuple(torch.from_numpy(t) for t in _part([[0.0, 0.0]], [[-1, -1]], [[-1, -1]]))
    value, level, box = api.combine_slices([a, b])
    assert isinstance(value, torch.Tensor)
    assert value.tolist() == [[2.0, 0.0]] and level.tolist() == [[1, -1]]
    assert box.tolist() == [[4, -1]]
    with pytest.raises(ValueError):
        api.combine_slices([])
    with pytest.raises(ValueError):
        api.combine_slices([a, _part([[0.0]], [[-1]], [[-1]])])
    with pytest.raises(ValueError):
        api.combine_slices([(a[0].float(), a[1], a[2])])
