"""What the product methods of runtime.Scene hand to the native library, and what they and the
api's *_scene functions refuse, without a device: the library is replaced by a recorder, the
context by a stand-in on the CPU.  Every valid call pins the entry point, its argument count, the
scalars, the host arrays behind the ctypes pointers, which pointers are null and the tensors that
come back; every invalid call pins the exact message and that nothing reached the library."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import _capi, api, runtime
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds

F64, I64, I32, I8, U8 = torch.float64, torch.int64, torch.int32, torch.int8, torch.uint8

INDEX = [[0, 0, 0], [2, 4, 6]]
RATIOS = [2]
SIZES = [[0.5, 0.25, 0.125], [0.25, 0.125, 0.0625]]
SIZES_X = [0.5, 0.25]
PROB_LO = [1.0, 2.0, 3.0]


class Recorder:
    """Stands in for the loaded library: every attribute is an entry point that records
    (name, args) and reports success."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


class FakeContext:
    device = torch.device("cpu")
    _check_tensor = runtime.Context._check_tensor

    def __init__(self):
        self._handle = C.c_void_p(0x1000)

    def join(self):
        pass

    def publish(self):
        pass


def make_scene(ctx, handle):
    scene = runtime.Scene.__new__(runtime.Scene)
    scene.ctx = ctx
    scene.boxes = [AmrBox((0, 0, 0), (1, 1, 1), None, 0, dims=(2, 2, 2)),
                   AmrBox((1, 0, 0), (2, 1, 1), None, 1, dims=(4, 4, 4))]
    scene._handle = C.c_void_p(handle)
    return scene


@pytest.fixture
def native(monkeypatch):
    recorder = Recorder()
    monkeypatch.setattr(_capi, "lib", lambda: recorder)
    return recorder


@pytest.fixture
def ctx():
    return FakeContext()


@pytest.fixture
def scene(ctx):
    made = make_scene(ctx, 0x2000)
    yield made
    made._handle = None                # nothing for Scene.__del__ to destroy


@pytest.fixture
def others(ctx):
    made = [make_scene(ctx, 0x3000 + 0x100 * i) for i in range(3)]
    yield made
    for one in made:
        one._handle = None


def only_call(native, name, count):
    assert len(native.calls) == 1
    got, args = native.calls[0]
    assert got == name and len(args) == count
    return args


def host(pointer, n, ctype):
    """The n values behind a typed ctypes pointer (or of a ctypes array)."""
    assert pointer._type_ is ctype
    return list(pointer[:n])


def null(argument):
    return argument is None or (isinstance(argument, C.c_void_p) and not argument.value)


def points_at(argument, tensor):
    return isinstance(argument, C.c_void_p) and argument.value == tensor.data_ptr() and \
        tensor.data_ptr() != 0


def is_tensor(t, shape, dtype):
    return isinstance(t, torch.Tensor) and tuple(t.shape) == tuple(shape) and \
        t.dtype == dtype and t.device == torch.device("cpu") and t.is_contiguous()


def all_equal(t, value):
    if isinstance(value, float) and math.isnan(value):
        return bool(torch.isnan(t).all())
    return bool((t == value).all())


def check_levels(args, at, with_sizes=True, with_origin=True):
    """index, ratios[, sizes, origin] from position `at`; returns the position behind them."""
    assert host(args[at], 6, C.c_int32) == [0, 0, 0, 2, 4, 6]
    assert host(args[at + 1], 1, C.c_int32) == [2]
    at += 2
    if with_sizes:
        assert host(args[at], 6, C.c_double) == [0.5, 0.25, 0.125, 0.25, 0.125, 0.0625]
        at += 1
    if with_origin:
        assert host(args[at], 3, C.c_double) == [1.0, 2.0, 3.0]
        at += 1
    return at


# ---- valid calls ---------------------------------------------------------------------------------

@pytest.mark.parametrize("given", [False, True])
def test_histogram(native, ctx, scene, given):
    counts = torch.full((2,), 7, dtype=I64) if given else None
    out = scene.histogram(ScalarTransform(), 0.25, 1.5, 2, counts)
    args = only_call(native, "avr_scene_histogram", 7)
    assert args[0] is ctx._handle and args[1] is scene._handle
    assert args[3:6] == (0.25, 1.5, 2)
    assert is_tensor(out, (2,), I64) and points_at(args[6], out)
    assert (out is counts and all_equal(out, 7)) if given else all_equal(out, 0)


def test_joint_histogram_alone(native, ctx, scene):
    cells, sums, totals = scene.joint_histogram([0.0, 1.0, 2.0])
    args = only_call(native, "avr_scene_joint_histogram", 12)
    assert args[0] is ctx._handle and args[1] is scene._handle
    assert args[2] is None and args[3] is None
    assert host(args[4], 3, C.c_double) == [0.0, 1.0, 2.0]
    assert args[5] == 2 and args[6] is None and args[7] == 1 and args[8] == 2
    assert is_tensor(cells, (2, 1, 2), I64) and all_equal(cells, 0) and points_at(args[9], cells)
    assert sums is None and args[10] is None
    assert is_tensor(totals, (2,), I64) and all_equal(totals, 0) and points_at(args[11], totals)


def test_joint_histogram_with_y_and_s(native, ctx, scene, others):
    y, s = others[:2]
    given = torch.full((3, 3, 2), 5, dtype=I64)
    cells, sums, totals = scene.joint_histogram(np.array([0, 1, 2]), y, (0.5, 1.5, 2.5, 3.5), s, 3,
                                                given)
    args = only_call(native, "avr_scene_joint_histogram", 12)
    assert args[2] is y._handle and args[3] is s._handle
    assert host(args[4], 3, C.c_double) == [0.0, 1.0, 2.0]
    assert host(args[6], 4, C.c_double) == [0.5, 1.5, 2.5, 3.5]
    assert args[5] == 2 and args[7] == 3 and args[8] == 3
    assert cells is given and all_equal(cells, 5) and points_at(args[9], cells)
    assert is_tensor(sums, (3, 3, 2), F64) and all_equal(sums, 0.0) and points_at(args[10], sums)
    assert is_tensor(totals, (2,), I64) and all_equal(totals, 0) and points_at(args[11], totals)


@pytest.mark.parametrize("indexed", [False, True])
def test_slice(native, ctx, scene, indexed):
    value, level, box = scene.slice((1, 2, 3), (0.5, 0, 0), (0, 0.25, 0), 3, 2,
                                    [5, 7] if indexed else None)
    args = only_call(native, "avr_slice_scene", 11)
    assert args[0] is ctx._handle and args[1] is scene._handle
    assert host(args[2], 3, C.c_double) == [1.0, 2.0, 3.0]
    assert host(args[3], 3, C.c_double) == [0.5, 0.0, 0.0]
    assert host(args[4], 3, C.c_double) == [0.0, 0.25, 0.0]
    assert args[5:7] == (3, 2)
    if indexed:
        assert host(args[7], 2, C.c_int32) == [5, 7]
    else:
        assert args[7] is None
    assert is_tensor(value, (2, 3), F64) and points_at(args[8], value)
    assert is_tensor(level, (2, 3), I8) and points_at(args[9], level)
    assert is_tensor(box, (2, 3), I32) and points_at(args[10], box)


def test_slice_into_given_tensors(native, ctx, scene):
    given = (torch.ones(6, dtype=F64), torch.ones((2, 3), dtype=I8), torch.ones((3, 2), dtype=I32))
    out = scene.slice((1, 2, 3), (0.5, 0, 0), (0, 0.25, 0), 3, 2, None, *given)
    args = only_call(native, "avr_slice_scene", 11)
    assert all(o is g and points_at(a, g) for o, g, a in zip(out, given, args[8:]))


@pytest.mark.parametrize("weighted", [False, True])
def test_axis_projection(native, ctx, scene, others, weighted):
    other = others[0] if weighted else None
    integral, weight, length = scene.axis_projection(2, (0.5, 1.5), 0.25, 0.125, 3, 2,
                                                     [0.5, 0.25], other)
    args = only_call(native, "avr_scene_axis_projection", 14)
    assert args[0] is ctx._handle and args[1] is scene._handle
    assert args[2] is (other._handle if weighted else None)
    assert args[3] == 2 and host(args[4], 2, C.c_double) == [0.5, 1.5]
    assert args[5:9] == (0.25, 0.125, 3, 2)
    assert host(args[9], 2, C.c_double) == [0.5, 0.25] and args[10] == 2
    assert is_tensor(integral, (2, 3), F64) and points_at(args[11], integral)
    assert is_tensor(length, (2, 3), F64) and points_at(args[13], length)
    if weighted:
        assert is_tensor(weight, (2, 3), F64) and points_at(args[12], weight)
    else:
        assert weight is None and args[12] is None


def test_derive(native, ctx, scene, others):
    origin = [[0.0, 0.5, 1.0], [1.5, 2.0, 2.5]]
    assert scene.derive(others[:2], [1, 2, 3], [0.5], origin, SIZES) is None
    args = only_call(native, "avr_scene_derive", 11)
    assert args[0] is ctx._handle and args[3] is scene._handle
    assert host(args[1], 2, C.c_void_p) == [0x3000, 0x3100] and args[2] == 2
    assert host(args[4], 3, C.c_uint32) == [1, 2, 3] and args[5] == 3
    assert host(args[6], 1, C.c_double) == [0.5] and args[7] == 1
    assert host(args[8], 6, C.c_double) == [0.0, 0.5, 1.0, 1.5, 2.0, 2.5]
    assert host(args[9], 6, C.c_double) == [0.5, 0.25, 0.125, 0.25, 0.125, 0.0625]
    assert args[10] == 2


def test_gradient(native, ctx, scene, others):
    assert scene.gradient(others[0], 1, INDEX, RATIOS, SIZES_X) is None
    args = only_call(native, "avr_scene_gradient", 8)
    assert args[0] is ctx._handle and args[1] is others[0]._handle and args[2] is scene._handle
    assert args[3] == 1
    assert check_levels(args, 4, with_sizes=False, with_origin=False) == 6
    assert host(args[6], 2, C.c_double) == [0.5, 0.25] and args[7] == 2


@pytest.mark.parametrize("given", [False, True])
def test_clumps(native, ctx, scene, others, given):
    count = torch.full((1,), 9, dtype=I64) if given else None
    out = scene.clumps(others[0], -1.5, math.inf, INDEX, RATIOS, count)
    args = only_call(native, "avr_scene_clumps", 9)
    assert args[0] is ctx._handle and args[1] is others[0]._handle and args[2] is scene._handle
    assert args[3:5] == (-1.5, math.inf)
    assert check_levels(args, 5, with_sizes=False, with_origin=False) == 7
    assert args[7] == 2
    assert is_tensor(out, (1,), I64) and points_at(args[8], out)
    assert (out is count and all_equal(out, 9)) if given else all_equal(out, 0)


def test_clumps_counts_levels_from_the_ratios(native, ctx, scene, others):
    scene.clumps(others[0], 0.0, 1.0, INDEX, [2, 2, 4])
    args = only_call(native, "avr_scene_clumps", 9)
    assert host(args[6], 3, C.c_int32) == [2, 2, 4] and args[7] == 4


@pytest.mark.parametrize("with_field", [False, True])
def test_clump_table(native, ctx, scene, others, with_field):
    field = others[0] if with_field else None
    cells, sums, totals = scene.clump_table(3, 2, field)
    args = only_call(native, "avr_scene_clump_table", 8)
    assert args[0] is ctx._handle and args[1] is scene._handle
    assert args[2] is (field._handle if with_field else None)
    assert args[3:5] == (3, 2)
    assert is_tensor(cells, (2, 3), I64) and all_equal(cells, 0) and points_at(args[5], cells)
    assert is_tensor(totals, (2,), I64) and all_equal(totals, 0) and points_at(args[7], totals)
    if with_field:
        assert is_tensor(sums, (2, 3), F64) and all_equal(sums, 0.0) and points_at(args[6], sums)
    else:
        assert sums is None and args[6] is None


@pytest.mark.parametrize("capacity, sampled", [(0, False), (0, True), (2, False), (2, True)])
def test_isosurface(native, ctx, scene, others, capacity, sampled):
    sample = others[0] if sampled else None
    counts, vertices, levels, samples = scene.isosurface(0.75, INDEX, RATIOS, SIZES, PROB_LO,
                                                         sample, capacity)
    args = only_call(native, "avr_scene_isosurface", 14)
    assert args[0] is ctx._handle and args[1] is scene._handle
    assert args[2] is (sample._handle if sampled else None)
    assert args[3] == 0.75 and check_levels(args, 4) == 8
    assert args[8:10] == (2, capacity)
    assert is_tensor(counts, (2,), I64) and all_equal(counts, 0) and points_at(args[13], counts)
    if capacity == 0:
        assert vertices is None and levels is None and samples is None
        assert all(null(a) for a in args[10:13])
        return
    assert is_tensor(vertices, (2, 3, 3), F64) and points_at(args[10], vertices)
    assert is_tensor(levels, (2,), U8) and points_at(args[11], levels)
    if sampled:
        assert is_tensor(samples, (2, 3), F64) and points_at(args[12], samples)
    else:
        assert samples is None and null(args[12])


def test_isosurface_adds_to_given_counts(native, ctx, scene):
    given = torch.full((2,), 4, dtype=I64)
    counts, _, _, _ = scene.isosurface(0.75, INDEX, RATIOS, SIZES, PROB_LO, None, 0, given)
    args = only_call(native, "avr_scene_isosurface", 14)
    assert counts is given and all_equal(counts, 4) and points_at(args[13], given)


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("as_tensor", [False, True])
def test_streamlines(native, ctx, scene, others, sampled, as_tensor):
    vy, vz, other = others
    seeds = np.array([[0.5, 1.0, 1.5], [2.0, 2.5, 3.0]])
    if as_tensor:
        seeds = torch.from_numpy(seeds)
    points, samples, counts, status = scene.streamlines(
        vy, vz, seeds, 0.5, -1, 1, INDEX, RATIOS, SIZES, PROB_LO, other if sampled else None)
    args = only_call(native, "avr_scene_streamlines", 19)
    assert args[0] is ctx._handle and args[1] is scene._handle
    assert args[2] is vy._handle and args[3] is vz._handle
    assert args[4] is (other._handle if sampled else None)
    # float64 contiguous seeds are used where they lie
    assert args[5].value == (seeds.data_ptr() if as_tensor else seeds.ctypes.data)
    assert args[6:10] == (2, 0.5, -1, 1)
    assert check_levels(args, 10) == 14 and args[14] == 2
    assert is_tensor(points, (2, 2, 3), F64) and all_equal(points, math.nan)
    assert is_tensor(counts, (2,), I32) and all_equal(counts, 0)
    assert is_tensor(status, (2,), U8) and all_equal(status, 0)
    assert points_at(args[15], points) and points_at(args[17], counts)
    assert points_at(args[18], status)
    if sampled:
        assert is_tensor(samples, (2, 2), F64) and all_equal(samples, math.nan)
        assert points_at(args[16], samples)
    else:
        assert samples is None and null(args[16])


@pytest.mark.parametrize("sampled", [False, True])
def test_streamlines_without_seeds(native, ctx, scene, others, sampled):
    vy, vz, other = others
    points, samples, counts, status = scene.streamlines(
        vy, vz, np.zeros((0, 3)), 0.5, 1, 1, INDEX, RATIOS, SIZES, PROB_LO,
        other if sampled else None)
    assert native.calls == []
    assert is_tensor(points, (0, 2, 3), F64) and is_tensor(counts, (0,), I32)
    assert is_tensor(status, (0,), U8)
    assert is_tensor(samples, (0, 2), F64) if sampled else samples is None


RAY_START = [[0.5, 1.0, 1.5], [2.0, 2.5, 3.0]]
RAY_END = [[3.5, 4.0, 4.5], [5.0, 5.5, 6.0]]


def check_ray_head(args, ctx, scene, start, end, max_trips):
    assert args[0] is ctx._handle and args[1] is scene._handle
    assert args[2].value == start.data_ptr() and args[3].value == end.data_ptr()
    assert args[4:6] == (2, max_trips)
    assert check_levels(args, 6) == 10 and args[10] == 2


def test_rays_count_pass(native, ctx, scene):
    start, end = torch.tensor(RAY_START, dtype=F64), torch.tensor(RAY_END, dtype=F64)
    counts, status, span = scene.rays(start, end, 5, INDEX, RATIOS, SIZES, PROB_LO)
    args = only_call(native, "avr_scene_rays", 22)
    check_ray_head(args, ctx, scene, start, end, 5)
    assert null(args[11]) and args[12] == 0
    assert is_tensor(counts, (2,), I32) and all_equal(counts, 0) and points_at(args[13], counts)
    assert is_tensor(status, (2,), U8) and all_equal(status, 3) and points_at(args[14], status)
    assert is_tensor(span, (2, 2), F64) and all_equal(span, math.nan) and points_at(args[15], span)
    assert all(null(a) for a in args[16:22])


@pytest.mark.parametrize("n_segments", [0, 3])
def test_rays_emit_pass(native, ctx, scene, n_segments):
    start, end = torch.tensor(RAY_START, dtype=F64), torch.tensor(RAY_END, dtype=F64)
    offsets = torch.tensor([0, 1, n_segments], dtype=I64)
    t0, t1, level, value, integral, covered = scene.rays(
        start, end, 2 ** 30, INDEX, RATIOS, SIZES, PROB_LO, offsets, n_segments)
    args = only_call(native, "avr_scene_rays", 22)
    check_ray_head(args, ctx, scene, start, end, 2 ** 30)
    assert points_at(args[11], offsets) and args[12] == n_segments
    assert all(null(a) for a in args[13:16])
    assert is_tensor(t0, (n_segments,), F64) and is_tensor(t1, (n_segments,), F64)
    assert is_tensor(level, (n_segments,), I8) and is_tensor(value, (n_segments,), F64)
    assert is_tensor(integral, (2,), F64) and all_equal(integral, 0.0)
    assert is_tensor(covered, (2,), F64) and all_equal(covered, 0.0)
    assert points_at(args[20], integral) and points_at(args[21], covered)
    if n_segments:
        assert all(points_at(a, t) for a, t in zip(args[16:20], (t0, t1, level, value)))
    else:                              # empty tensors have no address: null
        assert all(null(a) for a in args[16:20])


def test_rays_from_arrays(native, ctx, scene):
    start, end = np.array(RAY_START), np.array(RAY_END)
    scene.rays(start, end, 1, INDEX, RATIOS, SIZES, PROB_LO)
    args = only_call(native, "avr_scene_rays", 22)
    assert args[2].value == start.ctypes.data and args[3].value == end.ctypes.data
    assert args[4:6] == (2, 1)


@pytest.mark.parametrize("emit", [False, True])
def test_rays_without_rays(native, ctx, scene, emit):
    none = np.zeros((0, 3))
    if emit:
        out = scene.rays(none, none, 1, INDEX, RATIOS, SIZES, PROB_LO,
                         torch.zeros(1, dtype=I64), 0)
        shapes = [((0,), F64), ((0,), F64), ((0,), I8), ((0,), F64), ((0,), F64), ((0,), F64)]
    else:
        out = scene.rays(none, none, 1, INDEX, RATIOS, SIZES, PROB_LO)
        shapes = [((0,), I32), ((0,), U8), ((0, 2), F64)]
    assert native.calls == []
    assert len(out) == len(shapes)
    assert all(is_tensor(t, shape, dtype) for t, (shape, dtype) in zip(out, shapes))


@pytest.mark.parametrize("with_coverage", [False, True])
def test_covering_grid(native, ctx, scene, with_coverage):
    if with_coverage:
        values, coverage, cell_level = scene.covering_grid(1, (-1, 2, 3), (3, 2, 1), INDEX, RATIOS)
    else:
        values, coverage, cell_level = scene.covering_grid(1, (-1, 2, 3), (3, 2, 1), INDEX, RATIOS,
                                                           -2.5, False)
    args = only_call(native, "avr_scene_covering_grid", 12)
    assert args[0] is ctx._handle and args[1] is scene._handle and args[2] == 1
    assert host(args[3], 3, C.c_int32) == [-1, 2, 3] and host(args[4], 3, C.c_int32) == [3, 2, 1]
    assert check_levels(args, 5, with_sizes=False, with_origin=False) == 7
    assert args[7] == 2
    assert math.isnan(args[8]) if with_coverage else args[8] == -2.5
    assert is_tensor(values, (1, 2, 3), F64) and points_at(args[9], values)
    if with_coverage:
        assert is_tensor(coverage, (1, 2, 3), F64) and points_at(args[10], coverage)
        assert is_tensor(cell_level, (1, 2, 3), I8) and points_at(args[11], cell_level)
    else:
        assert coverage is None and cell_level is None
        assert null(args[10]) and null(args[11])


# ---- invalid calls: one wrong argument each -------------------------------------------------------

def bad(name, message, **changes):
    return pytest.param(name, changes, message, id=f"{name}-{'-'.join(changes)}")


FLAT6 = [0, 0, 0, 2, 4, 6]
WRONG_TYPE = "{} must be a contiguous {} tensor"

# name -> the keyword arguments of a valid call; "others" stands for other scenes
VALID = {
    "histogram": dict(transform=ScalarTransform(), range_min=0.0, range_max=1.0, bin_count=2),
    "joint_histogram": dict(x_edges=[0.0, 1.0, 2.0]),
    "slice": dict(origin=(0, 0, 0), du=(1, 0, 0), dv=(0, 1, 0), width=3, height=2),
    "axis_projection": dict(axis=0, origin_uv=(0, 0), du=1.0, dv=1.0, width=3, height=2,
                            level_dl=[0.5, 0.25]),
    "derive": dict(inputs=(), instructions=[1], constants=[0.5],
                   box_origin=[[0, 0, 0], [1, 1, 1]], level_cell_size=SIZES),
    "gradient": dict(field="other", axis=0, box_index_lo=INDEX, level_ratio=RATIOS,
                     level_cell_size=SIZES_X),
    "clumps": dict(field="other", lower=0.0, upper=1.0, box_index_lo=INDEX, level_ratio=RATIOS),
    "clump_table": dict(n_clumps=3, n_levels=2),
    "isosurface": dict(value=0.5, box_index_lo=INDEX, level_ratio=RATIOS, level_cell_size=SIZES,
                       prob_lo=PROB_LO),
    "streamlines": dict(vy="other", vz="other", seeds=RAY_START, step=0.5, direction=1,
                        max_steps=1, box_index_lo=INDEX, level_ratio=RATIOS,
                        level_cell_size=SIZES, prob_lo=PROB_LO),
    "rays": dict(start=RAY_START, end=RAY_END, max_trips=1, box_index_lo=INDEX,
                 level_ratio=RATIOS, level_cell_size=SIZES, prob_lo=PROB_LO),
    "covering_grid": dict(level=1, lo=(0, 0, 0), dims=(3, 2, 1), box_index_lo=INDEX,
                          level_ratio=RATIOS),
}

INDEX_MESSAGE = "box_index_lo must hold three values per box"
SIZES_MESSAGE = "level_cell_size must hold three values per level"
RATIO_MESSAGE = "level_ratio must hold one value per level transition"
ORIGIN_MESSAGE = "prob_lo must hold three values"

INVALID = [
    bad("histogram", "binCount must be positive", bin_count=0),
    bad("histogram", "counts has the wrong size", counts=torch.zeros(3, dtype=I64)),
    bad("histogram", WRONG_TYPE.format("counts", I64), counts=torch.zeros(2, dtype=I32)),
    bad("histogram", "counts must be a tensor on cpu", counts=np.zeros(2, dtype=np.int64)),
    bad("joint_histogram", "x_edges must hold at least two values", x_edges=[0.0]),
    bad("joint_histogram", "x_edges must hold at least two values", x_edges=[[0.0, 1.0]]),
    bad("joint_histogram", "y_edges must be given with y", y="other"),
    bad("joint_histogram", "y_edges must be given with y", y_edges=[0.0, 1.0]),
    bad("joint_histogram", "y_edges must hold at least two values", y="other", y_edges=[0.0]),
    bad("joint_histogram", "n_levels must be positive", n_levels=0),
    bad("joint_histogram", "cells must be [n_levels, ny, nx] and totals [2]",
        cells=torch.zeros((2, 2, 1), dtype=I64)),
    bad("joint_histogram", "cells must be [n_levels, ny, nx] and totals [2]",
        totals=torch.zeros(3, dtype=I64)),
    bad("joint_histogram", WRONG_TYPE.format("cells", I64),
        cells=torch.zeros((2, 1, 2), dtype=F64)),
    bad("joint_histogram", WRONG_TYPE.format("totals", I64), totals=torch.zeros(2, dtype=F64)),
    bad("joint_histogram", "sums must be [n_levels, ny, nx]", s="other",
        sums=torch.zeros((2, 2, 1), dtype=F64)),
    bad("joint_histogram", WRONG_TYPE.format("sums", F64), s="other",
        sums=torch.zeros((2, 1, 2), dtype=I64)),
    bad("slice", "image width and height must be positive", width=0),
    bad("slice", "image width and height must be positive", height=-1),
    bad("slice", "origin must hold three values", origin=(0, 0)),
    bad("slice", "du must hold three values", du=(1, 0, 0, 0)),
    bad("slice", "dv must hold three values", dv=()),
    bad("slice", "global_index must hold one entry per box of the scene", global_index=[0]),
    bad("slice", "value has the wrong size", value=torch.zeros((2, 2), dtype=F64)),
    bad("slice", "level has the wrong size", level=torch.zeros((3, 3), dtype=I8)),
    bad("slice", "box has the wrong size", box=torch.zeros(5, dtype=I32)),
    bad("slice", WRONG_TYPE.format("level", I8), level=torch.zeros((2, 3), dtype=I32)),
    bad("axis_projection", "axis must be 0 (x), 1 (y) or 2 (z)", axis=3),
    bad("axis_projection", "image width and height must be positive", width=0),
    bad("axis_projection", "origin_uv must hold two values", origin_uv=(0, 0, 0)),
    bad("axis_projection", "level_dl must hold one value per level", level_dl=[]),
    bad("axis_projection", "level_dl must hold one value per level", level_dl=[[0.5]]),
    bad("axis_projection", "weight is given exactly when weight_scene is",
        weight=torch.zeros((2, 3), dtype=F64)),
    bad("axis_projection", "integral has the wrong size", integral=torch.zeros((2, 2), dtype=F64)),
    bad("axis_projection", "weight has the wrong size", weight_scene="other",
        weight=torch.zeros((2, 2), dtype=F64)),
    bad("axis_projection", "length has the wrong size", length=torch.zeros(7, dtype=F64)),
    bad("axis_projection", WRONG_TYPE.format("length", F64), length=torch.zeros(6, dtype=I64)),
    bad("derive", "instructions and constants must be one-dimensional", instructions=[[1]]),
    bad("derive", "instructions and constants must be one-dimensional", constants=[[0.5]]),
    bad("derive", "box_origin must hold three values per box", box_origin=[[0, 0, 0]]),
    bad("derive", SIZES_MESSAGE, level_cell_size=SIZES_X),
    bad("derive", SIZES_MESSAGE, level_cell_size=np.zeros((0, 3))),
    bad("gradient", INDEX_MESSAGE, box_index_lo=FLAT6),
    bad("gradient", "level_cell_size must hold one value per level", level_cell_size=SIZES),
    bad("gradient", "level_cell_size must hold one value per level", level_cell_size=[]),
    bad("gradient", RATIO_MESSAGE, level_ratio=[2, 2]),
    bad("gradient", RATIO_MESSAGE, level_ratio=[[2]]),
    bad("clumps", INDEX_MESSAGE, box_index_lo=[[0, 0, 0]]),
    bad("clumps", RATIO_MESSAGE, level_ratio=[[2]]),
    bad("clumps", "count must hold one value", count=torch.zeros(2, dtype=I64)),
    bad("clumps", WRONG_TYPE.format("count", I64), count=torch.zeros(1, dtype=I32)),
    bad("clump_table", "n_clumps and n_levels must be at least 1", n_clumps=0),
    bad("clump_table", "n_clumps and n_levels must be at least 1", n_levels=0),
    bad("clump_table", "cells must be [n_levels, n_clumps] and totals hold two values",
        cells=torch.zeros((3, 2), dtype=I64)),
    bad("clump_table", "cells must be [n_levels, n_clumps] and totals hold two values",
        totals=torch.zeros(1, dtype=I64)),
    bad("clump_table", "sums must be [n_levels, n_clumps]", field="other",
        sums=torch.zeros((3, 2), dtype=F64)),
    bad("clump_table", "sums is given exactly when field is",
        sums=torch.zeros((2, 3), dtype=F64)),
    bad("isosurface", INDEX_MESSAGE, box_index_lo=FLAT6),
    bad("isosurface", SIZES_MESSAGE, level_cell_size=SIZES_X),
    bad("isosurface", RATIO_MESSAGE, level_ratio=[]),
    bad("isosurface", ORIGIN_MESSAGE, prob_lo=[0.0, 0.0]),
    bad("isosurface", "capacity must not be negative", capacity=-1),
    bad("isosurface", "counts must hold two values", counts=torch.zeros(3, dtype=I64)),
    bad("isosurface", WRONG_TYPE.format("counts", I64), counts=torch.zeros(2, dtype=F64)),
    bad("streamlines", INDEX_MESSAGE, box_index_lo=FLAT6),
    bad("streamlines", SIZES_MESSAGE, level_cell_size=[[0.5, 0.5]]),
    bad("streamlines", RATIO_MESSAGE, level_ratio=[2, 2]),
    bad("streamlines", ORIGIN_MESSAGE, prob_lo=[[0.0, 0.0, 0.0]]),
    bad("streamlines", "max_steps must not be negative", max_steps=-1),
    bad("streamlines", "seeds must hold three values per seed", seeds=torch.zeros((2, 2))),
    bad("streamlines", "seeds must hold three values per seed", seeds=torch.zeros(3)),
    bad("rays", INDEX_MESSAGE, box_index_lo=FLAT6),
    bad("rays", SIZES_MESSAGE, level_cell_size=SIZES_X),
    bad("rays", RATIO_MESSAGE, level_ratio=[]),
    bad("rays", ORIGIN_MESSAGE, prob_lo=[0.0]),
    bad("rays", "max_trips must lie in [1, 2^30]", max_trips=0),
    bad("rays", "max_trips must lie in [1, 2^30]", max_trips=2 ** 30 + 1),
    bad("rays", "n_segments must not be negative", n_segments=-1),
    bad("rays", "start and end must hold three values per ray", start=torch.zeros((2, 2))),
    bad("rays", "start and end must hold three values per ray", end=torch.zeros(3)),
    bad("rays", "start and end must hold the same number of rays", end=RAY_END[:1]),
    bad("rays", "offsets must hold n + 1 values", offsets=torch.zeros(2, dtype=I64)),
    bad("rays", WRONG_TYPE.format("offsets", I64), offsets=torch.zeros(3, dtype=I32)),
    bad("covering_grid", INDEX_MESSAGE, box_index_lo=FLAT6),
    bad("covering_grid", RATIO_MESSAGE, level_ratio=[[2]]),
    bad("covering_grid", "lo and dims must hold three values", lo=(0, 0)),
    bad("covering_grid", "lo and dims must hold three values", dims=(3, 2, 1, 1)),
    bad("covering_grid", "dims must be at least 1 (and lo and dims fit 32 bits)", dims=(3, 0, 1)),
    bad("covering_grid", "dims must be at least 1 (and lo and dims fit 32 bits)",
        dims=(2 ** 31, 1, 1)),
    bad("covering_grid", "dims must be at least 1 (and lo and dims fit 32 bits)",
        lo=(0, -2 ** 31, 0)),
    bad("covering_grid", "the region has 2^31 cells or more", dims=(2048, 2048, 512)),
]


@pytest.mark.parametrize("name, changes, message", INVALID)
def test_invalid_call(native, scene, others, name, changes, message):
    arguments = dict(VALID[name], **changes)
    arguments = {k: others[0] if isinstance(v, str) and v == "other" else v
                 for k, v in arguments.items()}
    with pytest.raises(ValueError) as raised:
        getattr(scene, name)(**arguments)
    assert str(raised.value) == message
    assert native.calls == []


@pytest.mark.parametrize("name", sorted(VALID))
def test_the_valid_calls_of_the_table_are_valid(native, scene, others, name):
    arguments = {k: others[0] if isinstance(v, str) and v == "other" else v
                 for k, v in VALID[name].items()}
    getattr(scene, name)(**arguments)
    assert len(native.calls) == 1


def test_the_first_wrong_level_argument_is_reported(native, scene):
    """index, sizes, ratios, prob_lo -- in this order, ahead of the method's own arguments."""
    wrong = dict(box_index_lo=FLAT6, level_cell_size=SIZES_X, level_ratio=[], prob_lo=[0.0])
    arguments = dict(VALID["rays"], max_trips=0, **wrong)
    for key, message in (("box_index_lo", INDEX_MESSAGE), ("level_cell_size", SIZES_MESSAGE),
                         ("level_ratio", RATIO_MESSAGE), ("prob_lo", ORIGIN_MESSAGE)):
        with pytest.raises(ValueError) as raised:
            scene.rays(**arguments)
        assert str(raised.value) == message
        arguments[key] = VALID["rays"][key]
    with pytest.raises(ValueError) as raised:
        scene.rays(**arguments)
    assert str(raised.value) == "max_trips must lie in [1, 2^30]"
    assert native.calls == []


# ---- api._level_setup and the *_scene functions, as far as they need no device --------------------

def geometry(local=2, levels=(0, 1), corner=0.0, world_scale=2.0):
    """A scene of len(levels) boxes, the first `local` of them on this rank.  With prob_lo =
    PROB_LO and SIZES the boxes start at the indices INDEX (level 1's along x moved by corner)."""
    starts = [(0.0, 0.0, 0.0), (0.5 + corner, 0.5, 0.375)]
    boxes = []
    for level, start in zip(levels, starts):
        low = tuple((PROB_LO[a] + start[a]) * world_scale for a in range(3))
        boxes.append(AmrBox(low, tuple(v + 1.0 for v in low), None, level, dims=(2, 2, 2)))
    out = api.SceneGeometry(boxes, boxes[:local], ScalarTransform(),
                            VolumeBounds((0, 0, 0), (1, 1, 1)))
    out.world_scale = world_scale
    return out


def test_level_setup():
    scene = geometry()
    sizes, ratios, index = api._level_setup(scene, scene.local_boxes, np.array(SIZES), PROB_LO,
                                            [2, 4, 4])
    assert sizes == [(0.5, 0.25, 0.125), (0.25, 0.125, 0.0625)]
    assert all(type(v) is float for c in sizes for v in c)
    assert ratios == [2] and type(ratios[0]) is int
    assert index.dtype == np.int32 and index.tolist() == INDEX


CELL_SIZES_MESSAGE = ("cell_sizes must hold (dx, dy, dz) per level up to the finest loaded one "
                      "(at most 16)")

LEVEL_SETUP_INVALID = [
    pytest.param(dict(cell_sizes=SIZES[:1]), CELL_SIZES_MESSAGE, id="too-few-sizes"),
    pytest.param(dict(cell_sizes=[SIZES[0]] * 17, ref_ratio=[2] * 16), CELL_SIZES_MESSAGE,
                 id="too-many-sizes"),
    pytest.param(dict(cell_sizes=[SIZES[0], (0.25, 0.125)]), CELL_SIZES_MESSAGE,
                 id="two-values"),
    pytest.param(dict(ref_ratio=[]), "ref_ratio must hold one ratio per level transition",
                 id="too-few-ratios"),
    pytest.param(dict(corner=0.125), "box 1: its low corner along axis 0 is at index 2.5 of "
                 "level 1, which is not an integer", id="corner"),
]


@pytest.mark.parametrize("changes, message", LEVEL_SETUP_INVALID)
def test_level_setup_invalid(changes, message):
    changes = dict(changes)
    scene = geometry(corner=changes.pop("corner", 0.0))
    arguments = dict(cell_sizes=SIZES, prob_lo=PROB_LO, ref_ratio=RATIOS)
    arguments.update(changes)
    with pytest.raises(ValueError) as raised:
        api._level_setup(scene, scene.local_boxes, **arguments)
    assert str(raised.value) == message


class NoDevice:
    """A context that must not be reached."""

    def __getattr__(self, name):
        raise AssertionError(f"the context was used ({name})")


LEVELS = dict(cell_sizes=SIZES, prob_lo=PROB_LO, ref_ratio=RATIOS)
SCENE_CALLS = {
    "gradient_scene": dict(axis=0, **LEVELS),
    "clump_scene": dict(lower=0.0, upper=1.0, **LEVELS),
    "isosurface_scene": dict(value=0.5, **LEVELS),
    "streamline_scene": dict(seeds=RAY_START, **LEVELS),
    "covering_grid_scene": dict(level=1, lo=(0, 0, 0), dims=(3, 2, 1), **LEVELS),
    "ray_scene": dict(start=RAY_START, end=RAY_END, **LEVELS),
}
ONE_RANK = {
    "gradient_scene": "a gradient field needs every box of the scene on one rank: "
                      "ghost cells are not exchanged between ranks",
    "clump_scene": "clumps need every box of the scene on one rank: "
                   "labels are not merged between ranks",
    "isosurface_scene": "an isosurface needs every box of the scene on one rank: "
                        "ghost cells are not exchanged between ranks",
    "streamline_scene": "streamlines need every box of the scene on one rank: "
                        "lines are not handed over between ranks",
    "covering_grid_scene": "a covering grid needs every box of the scene on one rank: "
                           "cells are not gathered between ranks",
    "ray_scene": "rays need every box of the scene on one rank: "
                 "rays are not handed over between ranks",
}


def call_scene_function(name, scene, changes):
    arguments = dict(SCENE_CALLS[name], **changes)
    if name == "streamline_scene":
        return api.streamline_scene(NoDevice(), scene, arguments.pop("vy", scene),
                                    arguments.pop("vz", scene), **arguments)
    return getattr(api, name)(NoDevice(), scene, **arguments)


@pytest.mark.parametrize("split", ["ranks", "boxes"])
@pytest.mark.parametrize("name", sorted(SCENE_CALLS))
def test_scene_functions_need_one_rank(name, split):
    scene = geometry(local=2 if split == "ranks" else 1)
    with pytest.raises(NotImplementedError) as raised:
        call_scene_function(name, scene, dict(n_ranks=2) if split == "ranks" else {})
    assert str(raised.value) == ONE_RANK[name]


def scene_bad(name, message, **changes):
    return pytest.param(name, changes, message, id=f"{name}-{'-'.join(changes)}")


SCENE_INVALID = [
    scene_bad("gradient_scene", "axis must be 0 (x), 1 (y) or 2 (z)", axis=3),
    scene_bad("gradient_scene", CELL_SIZES_MESSAGE, cell_sizes=SIZES[:1]),
    scene_bad("gradient_scene", "ref_ratio must hold one ratio per level transition",
              ref_ratio=[]),
    scene_bad("clump_scene", CELL_SIZES_MESSAGE, cell_sizes=SIZES[:1]),
    scene_bad("isosurface_scene", "an isosurface's value must be finite", value=math.inf),
    scene_bad("isosurface_scene", "the sample scene must hold the same boxes as the scene",
              sample=geometry(local=1)),
    scene_bad("isosurface_scene", CELL_SIZES_MESSAGE, cell_sizes=SIZES[:1]),
    scene_bad("streamline_scene", "step must be finite and lie in (0, 1]", step=0.0),
    scene_bad("streamline_scene", "step must be finite and lie in (0, 1]", step=math.nan),
    scene_bad("streamline_scene", "direction must be +1 or -1", direction=0),
    scene_bad("streamline_scene", "max_steps must lie in [0, 2^20]", max_steps=2 ** 20 + 1),
    scene_bad("streamline_scene", "the scenes must hold the same boxes", vz=geometry(local=1)),
    scene_bad("streamline_scene", "the scenes must hold the same boxes",
              sample=geometry(local=1)),
    scene_bad("streamline_scene", "seeds must be an array [n, 3]", seeds=[0.0, 0.0, 0.0]),
    scene_bad("streamline_scene", "n_seeds * (max_steps + 1) must stay below 2^32",
              seeds=np.zeros((2 ** 12, 3)), max_steps=2 ** 20),
    scene_bad("streamline_scene", CELL_SIZES_MESSAGE, cell_sizes=SIZES[:1]),
    scene_bad("covering_grid_scene", "lo and dims must hold three values", lo=(0, 0)),
    scene_bad("covering_grid_scene", "dims must be at least 1", dims=(3, 0, 1)),
    scene_bad("covering_grid_scene", "level must lie in [0, the number of cell_sizes)", level=2),
    scene_bad("covering_grid_scene", CELL_SIZES_MESSAGE, cell_sizes=SIZES[:1], level=0),
    scene_bad("ray_scene", CELL_SIZES_MESSAGE, cell_sizes=SIZES[:1]),
    scene_bad("ray_scene", "max_trips must lie in [1, 2^30]", max_trips=0),
    scene_bad("ray_scene", "max_trips must lie in [1, 2^30]", max_trips=2 ** 30 + 1),
]


@pytest.mark.parametrize("name, changes, message", SCENE_INVALID)
def test_scene_functions_invalid(name, changes, message):
    with pytest.raises(ValueError) as raised:
        call_scene_function(name, geometry(), changes)
    assert str(raised.value) == message


def test_derive_scene_invalid():
    scene = geometry()
    program = types.SimpleNamespace(fields=("a",))
    for scenes, target, sizes, message in (
            ([], scene, SIZES, "scenes must hold one loaded scene per field of the program"),
            ([geometry(local=1)], scene, SIZES, "the scenes must hold the same boxes as geometry"),
            ([scene], scene, SIZES[:1], CELL_SIZES_MESSAGE),
            ([scene], scene, [SIZES[0], (0.25,)], CELL_SIZES_MESSAGE)):
        with pytest.raises(ValueError) as raised:
            api.derive_scene(NoDevice(), program, scenes, target, sizes)
        assert str(raised.value) == message
