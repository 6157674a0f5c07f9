"""What runtime.Scene.ray_sums hands to the native library and what it refuses, without a device:
the recorder and the stand-ins of test_scene_arguments.py.  The valid calls pin the entry point,
its 19 arguments, which pointers are null and the tensors that come back; the invalid ones the exact
message and that nothing reached the library."""
import math

import numpy as np
import pytest
import torch

from test_scene_arguments import (F64, I32, INDEX, PROB_LO, RATIO_MESSAGE, RATIOS, RAY_END,
                                  RAY_START, SIZES, U8, all_equal, check_levels, ctx, is_tensor,
                                  native, null, only_call, others, points_at,
                                  scene)  # noqa: F401  (fixtures among them)


@pytest.mark.parametrize("weighted", [False, True])
def test_ray_sums(native, ctx, scene, others, weighted):
    start, end = torch.tensor(RAY_START, dtype=F64), torch.tensor(RAY_END, dtype=F64)
    weight = others[0] if weighted else None
    counts, status, span, integral, weight_sum, counted, covered = scene.ray_sums(
        start, end, 5, INDEX, RATIOS, SIZES, PROB_LO, weight)
    args = only_call(native, "avr_scene_ray_sums", 19)
    assert args[0] is ctx._handle and args[1] is scene._handle
    assert args[2] is (weight._handle if weighted else None)
    assert args[3].value == start.data_ptr() and args[4].value == end.data_ptr()
    assert args[5:7] == (2, 5)
    assert check_levels(args, 7) == 11 and args[11] == 2
    assert is_tensor(counts, (2,), I32) and all_equal(counts, 0) and points_at(args[12], counts)
    assert is_tensor(status, (2,), U8) and all_equal(status, 3) and points_at(args[13], status)
    assert is_tensor(span, (2, 2), F64) and all_equal(span, math.nan) and points_at(args[14], span)
    assert is_tensor(integral, (2,), F64) and all_equal(integral, 0.0)
    assert points_at(args[15], integral)
    if weighted:
        assert is_tensor(weight_sum, (2,), F64) and all_equal(weight_sum, 0.0)
        assert points_at(args[16], weight_sum)
    else:
        assert weight_sum is None and null(args[16])
    assert is_tensor(counted, (2,), F64) and all_equal(counted, 0.0) and points_at(args[17], counted)
    assert is_tensor(covered, (2,), F64) and all_equal(covered, 0.0) and points_at(args[18], covered)
    assert len({t.data_ptr() for t in (integral, counted, covered)}) == 3


def test_ray_sums_from_arrays_and_without_rays(native, ctx, scene, others):
    start, end = np.array(RAY_START), np.array(RAY_END)
    scene.ray_sums(start, end, 2 ** 30, INDEX, RATIOS, SIZES, PROB_LO)
    args = only_call(native, "avr_scene_ray_sums", 19)
    assert args[3].value == start.ctypes.data and args[4].value == end.ctypes.data
    assert args[5:7] == (2, 2 ** 30)
    native.calls.clear()
    none = np.zeros((0, 3))
    out = scene.ray_sums(none, none, 1, INDEX, RATIOS, SIZES, PROB_LO, others[1])
    assert native.calls == []                          # nothing to launch
    shapes = [((0,), I32), ((0,), U8), ((0, 2), F64)] + [((0,), F64)] * 4
    assert len(out) == 7 and all(is_tensor(t, *shape) for t, shape in zip(out, shapes))
    assert scene.ray_sums(none, none, 1, INDEX, RATIOS, SIZES, PROB_LO)[4] is None


def test_ray_sums_refusals(native, ctx, scene, others):
    valid = dict(start=RAY_START, end=RAY_END, max_trips=1, box_index_lo=INDEX, level_ratio=RATIOS,
                 level_cell_size=SIZES, prob_lo=PROB_LO)
    elsewhere = others[2]
    elsewhere.ctx = object()
    wrong = [
        (dict(max_trips=0), "max_trips must lie in [1, 2^30]"),
        (dict(max_trips=2 ** 30 + 1), "max_trips must lie in [1, 2^30]"),
        (dict(start=torch.zeros((2, 2))), "start and end must hold three values per ray"),
        (dict(end=torch.zeros(3)), "start and end must hold three values per ray"),
        (dict(end=RAY_END[:1]), "start and end must hold the same number of rays"),
        (dict(weight=elsewhere), "the weight scene belongs to another context"),
        (dict(level_ratio=[]), RATIO_MESSAGE),
    ]
    for arguments, message in wrong:
        with pytest.raises(ValueError) as raised:
            scene.ray_sums(**{**valid, **arguments})
        assert str(raised.value) == message, arguments
    assert native.calls == []
    elsewhere.ctx = ctx
