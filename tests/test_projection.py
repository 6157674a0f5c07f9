"""Column projections, what needs no GPU: the C ABI's new entries, the ABI version, the unchanged
render modes and the argument checks of api.project (raised before any GPU work)."""
import inspect

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, runtime
from amrvolumerenderer_amd.renderer import FrameRenderer

NEW_SYMBOLS = ["avr_paint_box_projection", "avr_render_plan_projection",
               "avr_march_plan_projection", "avr_fold_plan_projection",
               "avr_fold_plan_own_projection", "avr_fold_plan_image_projection",
               "avr_renderer_render_projection", "avr_projection_colorize"]


def test_new_symbols_resolve_in_the_library():
    handle = _capi.lib()
    for name in NEW_SYMBOLS:
        assert getattr(handle, name) is not None, name
        assert name in _capi.SIGNATURES, name


def test_abi_version_stays_two():
    assert _capi.lib().avr_abi_version() == 2


def test_render_modes_are_unchanged():
    assert api.RenderOptions().mode == "volume"
    assert api.RENDER_MODES == ("volume", "max_intensity")
    assert inspect.signature(api.render).parameters["mode"].default == "volume"
    assert "quantity" not in inspect.signature(api.render).parameters
    assert hasattr(FrameRenderer, "render_projection")
    assert runtime.PROJECTION_QUANTITIES == ("column", "mean")


@pytest.mark.parametrize("kwargs,match", [
    (dict(quantity="density"), "quantity"),
    (dict(quantity="Column"), "quantity"),
    (dict(value_range=(2.0, 1.0)), "lo < hi"),
    (dict(value_range=(1.0, 1.0)), "lo < hi"),
    (dict(value_range=(0.0, float("inf"))), "finite"),
    (dict(value_range=(float("nan"), 1.0)), "finite"),
    (dict(value_range=(1.0,)), "two values"),
    (dict(value_range=(0.0, 1.0), log_scale=True), "positive"),
    (dict(value_range=(-1.0, 1.0), log_scale=True), "positive"),
    (dict(width=0), "dimensions"),
])
def test_bad_arguments_are_refused_before_any_gpu_work(tmp_path, kwargs, match, monkeypatch):
    # no plotfile, and no runtime: the error comes first
    def no_gpu(*args, **kw):
        raise AssertionError("GPU work started")
    monkeypatch.setattr(api, "_runtime_scope", no_gpu)
    with pytest.raises(ValueError, match=match):
        api.project(str(tmp_path / "missing"), **kwargs)


def test_good_arguments_pass_the_checks():
    assert api.validate_projection_arguments(8, 8, "mean", True, (0.5, 2.0)) == (0.5, 2.0)
    assert api.validate_projection_arguments(8, 8, "column", False, None) is None
    assert api.validate_projection_arguments(8, 8, "column", False, [-1, 1]) == (-1.0, 1.0)


def test_rgb_table_is_the_colour_maps_bytes():
    table = api.projection_rgb_table([(0.0, 0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 0.5, 0.25, 1.0)])
    assert table.shape == (256, 3) and table.dtype == np.uint8
    assert tuple(table[0]) == (0, 0, 0)
    assert tuple(table[255]) == (255, 128, 64)
    assert np.all(np.diff(table[:, 0].astype(int)) >= 0)
    with pytest.raises(ValueError, match="entries"):
        api.projection_rgb_table([(0.0, 1.0)])
