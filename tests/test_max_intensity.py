"""Maximum-intensity projection frames, what needs no GPU: the C ABI's new entries, the ABI version,
and the Python surface's mode handling (unchanged defaults, errors before any GPU work)."""
import ctypes as C
import inspect

import pytest

from amrvolumerenderer_amd import _capi, api
from amrvolumerenderer_amd.renderer import FrameRenderer

NEW_SYMBOLS = ["avr_paint_box_max", "avr_render_plan_max", "avr_march_plan_max",
               "avr_fold_plan_max", "avr_fold_plan_own_max", "avr_fold_plan_image_max",
               "avr_renderer_render_max"]


def test_new_symbols_resolve_in_the_library():
    handle = C.CDLL(_capi.library_path()) if hasattr(_capi, "library_path") else _capi.lib()
    for name in NEW_SYMBOLS:
        assert getattr(handle, name) is not None, name


def test_abi_version_stays_two():
    assert _capi.lib().avr_abi_version() == 2


def test_defaults_are_unchanged():
    assert api.RenderOptions().mode == "volume"
    assert inspect.signature(api.render).parameters["mode"].default == "volume"
    assert api.RENDER_MODES == ("volume", "max_intensity")
    assert hasattr(FrameRenderer, "render_max_intensity")


@pytest.mark.parametrize("mode", ["max", "MIP", "", "Volume"])
def test_bad_modes_are_refused_before_any_gpu_work(mode, tmp_path):
    with pytest.raises(ValueError, match="mode"):
        api.validate_options(api.RenderOptions(mode=mode))
    with pytest.raises(ValueError, match="mode"):
        api.render(str(tmp_path / "missing"), mode=mode)
    with pytest.raises(ValueError, match="mode"):
        api.run(str(tmp_path / "missing"), api.RenderOptions(mode=mode))
    with pytest.raises(ValueError, match="mode"):
        api.render_amr_data(None, api.RenderOptions(mode=mode))


def test_mip_with_antialiasing_is_refused(tmp_path):
    with pytest.raises(ValueError, match="antialiasing"):
        api.validate_options(api.RenderOptions(mode="max_intensity", antialiasing=4))
    with pytest.raises(ValueError, match="antialiasing"):
        api.render(str(tmp_path / "missing"), antialiasing=4, mode="max_intensity")
    api.validate_options(api.RenderOptions(mode="max_intensity"))
