"""On-axis projections without a GPU: the numpy reference against a brute-force loop,
conservation, the argument checks of api.project_axis, combine_axis_projections and the new
symbol's declaration and binding."""
import math
import os

import numpy as np
import pytest

from amrvolumerenderer_amd import _capi, api, runtime

import axis_projection_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROB_LO = (0.0, -1.0, 2.0)
PROB_HI = (2.0, 0.5, 3.0)      # 4 x 3 x 2 coarse cells of 0.5: every size is a power of two


def tiny_levels():
    """4 x 3 x 2 coarse cells, one 4 x 2 x 4 fine grid over two coarse columns; small integers with
    a NaN, a +Inf and a -Inf in each field."""
    rng = np.random.default_rng(11)
    boxes = [[((0, 0, 0), (3, 2, 1))], [((2, 2, 0), (5, 3, 3))]]
    domains = [((0, 0, 0), (3, 2, 1)), ((0, 0, 0), (7, 5, 3))]
    levels = []
    for d, bs in zip(domains, boxes):
        data = []
        for lo, hi in bs:
            shape = (2, hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
            cells = rng.integers(-1000, 1001, size=shape).astype(np.float64)
            for comp in range(2):
                flat = cells[comp].reshape(-1)
                flat[rng.choice(flat.size, 3, replace=False)] = [np.nan, np.inf, -np.inf]
            data.append(cells)
        levels.append({"domain": d, "boxes": bs, "data": data})
    return levels


def whole_domain(axis):
    au, av = ref.image_axes(axis)
    center = tuple(0.5 * (PROB_LO[a] + PROB_HI[a]) for a in range(3))
    return center, (PROB_HI[au] - PROB_LO[au], PROB_HI[av] - PROB_LO[av])


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("w", [None, 1])
def test_reference_equals_the_brute_force_loop(axis, w):
    levels = tiny_levels()
    center, widths = whole_domain(axis)
    dl = [c[axis] for c in ref.cell_sizes(levels, PROB_LO, PROB_HI)]
    au, av = ref.image_axes(axis)
    # three pixels per finest cell: no line on a face
    width = 3 * (levels[-1]["domain"][1][au] + 1)
    height = 3 * (levels[-1]["domain"][1][av] + 1)
    assert ref.clearance(levels, PROB_LO, PROB_HI, center, widths, width, height, axis) > 0.1
    got = ref.reference(levels, PROB_LO, PROB_HI, axis, 0, w, center, widths, width, height, dl,
                        with_fsum=True)
    integral, weight, length = ref.brute_force(levels, PROB_LO, PROB_HI, axis, 0, w, center,
                                               widths, width, height, dl)
    # integers and power-of-two sizes: every sum is exact in any order
    assert np.array_equal(got["integral"], integral) and np.array_equal(got["length"], length)
    assert np.array_equal(got["weight"], weight)
    assert np.array_equal(got["integral_fsum"], integral)
    assert np.array_equal(got["weight_fsum"], weight)
    assert (got["count"] > 0).all() and (length > 0).all()
    assert (got["integral_abs"] >= np.abs(integral)).all()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_conservation_of_the_volume_integral(axis):
    """Pixels equal to the finest cell's footprint over the whole domain: the sum of integral *
    pixel area is the volume integral of the field over the uncovered finite cells."""
    levels = tiny_levels()
    center, widths = whole_domain(axis)
    sizes = ref.cell_sizes(levels, PROB_LO, PROB_HI)
    dl = [c[axis] for c in sizes]
    au, av = ref.image_axes(axis)
    width = levels[-1]["domain"][1][au] + 1
    height = levels[-1]["domain"][1][av] + 1
    got = ref.reference(levels, PROB_LO, PROB_HI, axis, 0, None, center, widths, width, height, dl)
    area = sizes[-1][au] * sizes[-1][av]
    total = math.fsum((got["integral"] * area).reshape(-1).tolist())
    want = []
    for level in range(len(levels)):
        term, _, counts = ref.level_terms(levels, level, len(levels) - 1, 0, None)
        vol = sizes[level][0] * sizes[level][1] * sizes[level][2]
        want.extend((term[counts] * vol).tolist())
    want = math.fsum(want)
    assert len(levels) == 2 and want != 0.0
    assert abs(total - want) <= 2.0 ** -52 * abs(want)


def test_every_argument_check_comes_before_the_plotfile_is_opened():
    missing = "/nonexistent/plotfile"
    bad = [
        dict(axis="w"), dict(axis=2), dict(quantity="sum"), dict(width=0), dict(height=-3),
        dict(center=(0.0, 1.0)), dict(center=(0.0, float("nan"), 1.0)),
        dict(center=(0.0, float("inf"), 1.0)),
        dict(plane_width=(1.0,)), dict(plane_width=(1.0, 0.0)), dict(plane_width=(-1.0, 1.0)),
        dict(plane_width=(1.0, float("inf"))),
        dict(value_range=(1.0,)), dict(value_range=(2.0, 1.0)),
        dict(value_range=(0.0, float("nan"))), dict(value_range=(0.0, 1.0), log_scale=True),
        dict(weight=""), dict(weight=3, quantity="mean"),
        dict(weight="density"), dict(weight="density", quantity="column"),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            api.project_axis(missing, **kw)
    # ... and what is in order reaches the file system
    for kw in (dict(), dict(weight="density", quantity="mean"), dict(axis="x", quantity="mean")):
        with pytest.raises(RuntimeError, match="does not exist"):
            api.project_axis(missing, **kw)
    assert api.AXIS_PROJECTION_QUANTITIES == ("column", "mean")
    center, widths, rng = api.validate_axis_projection_arguments(
        8, 4, "y", "mean", (1, 2, 3), (4, 5), True, (1, 10), "w")
    assert center == (1.0, 2.0, 3.0) and widths == (4.0, 5.0) and rng == (1.0, 10.0)
    assert api.validate_axis_projection_arguments(8, 4) == (None, None, None)


def test_combine_axis_projections():
    rng = np.random.default_rng(3)
    parts = [tuple(rng.standard_normal((5, 7)) for _ in range(3)) for _ in range(3)]
    keep = [tuple(a.copy() for a in p) for p in parts]
    integral, weight, length = api.combine_axis_projections(parts)
    for got, k in zip((integral, weight, length), range(3)):
        assert np.array_equal(got, (keep[0][k] + keep[1][k]) + keep[2][k])
    assert all(np.array_equal(a, b) for p, q in zip(parts, keep) for a, b in zip(p, q))
    unweighted = [(p[0], None, p[2]) for p in parts]
    assert api.combine_axis_projections(unweighted)[1] is None
    assert np.array_equal(api.combine_axis_projections(parts[:1])[0], parts[0][0])
    with pytest.raises(ValueError):
        api.combine_axis_projections([])
    with pytest.raises(ValueError):
        api.combine_axis_projections([parts[0], unweighted[1]])
    with pytest.raises(ValueError):
        api.combine_axis_projections([parts[0], tuple(a[:4] for a in parts[1])])
    import torch
    tensors = [tuple(torch.from_numpy(a.copy()) for a in p) for p in parts]
    got = api.combine_axis_projections(tensors)
    assert np.array_equal(got[0].numpy(), integral) and np.array_equal(got[2].numpy(), length)


def test_the_header_declares_the_symbol_and_the_binding_resolves():
    header = open(os.path.join(ROOT, "include", "avr_hip.h")).read()
    assert "int avr_scene_axis_projection(avr_context *ctx, const avr_scene *scene_f" in header
    assert "avr_scene_axis_projection" in _capi.SIGNATURES
    assert len(_capi.SIGNATURES["avr_scene_axis_projection"][1]) == 14
    assert getattr(_capi.lib(), "avr_scene_axis_projection") is not None
    assert _capi.lib().avr_abi_version() == 2
    assert hasattr(runtime.Scene, "axis_projection")
    for name in ("project_axis", "project_axis_scene", "combine_axis_projections",
                 "validate_axis_projection_arguments"):
        assert callable(getattr(api, name))
