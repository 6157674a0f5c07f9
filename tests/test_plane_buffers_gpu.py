"""The context's grow-only plane buffers (the on-axis projection's partial planes, the gradient's
face planes) across a regrow: one context runs both products on a small scene, on a larger one --
two boxes of 130 cells along x, so two segments per column and more faces: both buffers grow -- and
on the small one again, which re-uses the grown buffers.  Every result has the bits of the same
call on a context of its own, whose buffers have exactly the call's size."""
import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import runtime
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform

pytestmark = pytest.mark.gpu

AXIS = 0          # along x: the image axes are (y, z)
CELL = 0.125
# (nx, ny, nz) and the first cell's index of every box
SMALL = [((4, 4, 4), (0, 0, 0))]
LARGE = [((130, 8, 8), (0, 0, 0)), ((130, 8, 8), (0, 8, 0))]


def _products(ctx, spec, seed):
    """(integral, length, [gradient of every box]) of the scene on ctx, as numpy arrays."""
    rng = np.random.default_rng(seed)
    fields, outs = [], []
    for dims, lo in spec:
        lo_corner = tuple(CELL * i for i in lo)
        hi_corner = tuple(CELL * (i + n) for i, n in zip(lo, dims))
        cells = torch.from_numpy(rng.standard_normal(dims[::-1])).to(ctx.device)
        fields.append(AmrBox(lo_corner, hi_corner, cells, 0))
        outs.append(AmrBox(lo_corner, hi_corner, torch.zeros_like(cells), 0))
    field = ctx.create_scene(fields, ScalarTransform())
    out = ctx.create_scene(outs, ScalarTransform())
    width = sum(dims[1] for dims, _ in spec)
    height = spec[0][0][2]
    integral, _, length = field.axis_projection(AXIS, (0.0, 0.0), CELL, CELL, width, height, [CELL])
    out.gradient(field, AXIS, [lo for _, lo in spec], [], [CELL])
    ctx.synchronize()
    return (integral.cpu().numpy(), length.cpu().numpy(), [b.values.cpu().numpy() for b in outs])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_results_are_the_same_bits_before_across_and_after_a_regrow():
    shared = runtime.Context(0)
    for step, spec in enumerate([SMALL, LARGE, SMALL]):
        got = _products(shared, spec, 50 + step)
        fresh = runtime.Context(0)
        want = _products(fresh, spec, 50 + step)
        fresh.close()
        assert np.count_nonzero(want[0]) == want[0].size and np.all(want[1] > 0.0)  # every pixel is covered
        assert all(np.count_nonzero(g) > 0 for g in want[2])
        assert _same_bits(got[0], want[0]) and _same_bits(got[1], want[1]), step
        assert len(got[2]) == len(want[2]) == len(spec)
        for g, w in zip(got[2], want[2]):
            assert _same_bits(g, w), step
    shared.close()
