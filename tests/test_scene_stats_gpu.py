"""scalar_stats_kernel and histogram_kernel (avr_scene_stats.hip) at their layout edges: both load
paths of for_each_cell with the pair path's single-cell tail, scans that loop, reads outside a view
(the storages around the views are poison), all four histogram instantiations with ranges that
clamp, cells on bin edges, value edges of the statistics, and the reductions over ranks.

Every comparison is against the CPU oracle and plain numpy (tests/scene_stats_cases.py, held to
its claims by tests/test_scene_stats_cases.py), with == throughout: the results are minima, maxima
and integer counts.  Log-scale inputs go through cases.log_safe first, which keeps every cell away
from the bin edges by more than the last bit of log() can move it."""
import os
import sys

import numpy as np
import pytest
import torch

from amrvolumerenderer_amd import api, runtime
from amrvolumerenderer_amd.types import AmrBox, ScalarTransform, VolumeBounds

import scene_stats_cases as cases
from helpers import spawn_ranks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NOTHING = (INF, -INF, INF, 0)
CORNERS = ((0, 0, 0), (1, 1, 1))


def _device_boxes(device, case):
    """The case's boxes in HBM: every storage uploaded once, every view taken as on the host, and
    the alignment that the case claims asserted on the device pointers and strides."""
    uploaded, boxes = {}, []
    for storage, view in case.boxes:
        if id(storage) not in uploaded:
            uploaded[id(storage)] = torch.from_numpy(storage).to(device)
        t = uploaded[id(storage)]
        assert t.data_ptr() % 16 == 0
        if view is None:
            values, (offset, shape, strides) = t, (0, storage.shape, tuple(
                s // 8 for s in storage.strides))
        else:
            offset, shape, strides = view
            values = torch.as_strided(t, shape, strides, offset)
        assert tuple(values.shape) == tuple(shape)
        assert values.data_ptr() % 16 == 8 * (offset % 2)
        assert values.stride(0) % 2 == strides[0] % 2 and values.stride(1) % 2 == strides[1] % 2
        assert shape[2] == 1 or values.stride(2) == 1
        paired = (values.data_ptr() % 16 == 0 and values.stride(0) % 2 == 0 and
                  values.stride(1) % 2 == 0)
        assert paired == cases.is_paired(offset, strides[1], strides[0])
        boxes.append(AmrBox(CORNERS[0], CORNERS[1], values))
    return boxes


def _oracle_boxes(O, case):
    return [O.make_box(v, *CORNERS) for v in cases.case_views(case)]


def _copy(case):
    copies = {}
    for storage, _ in case.boxes:
        if id(storage) not in copies:
            copies[id(storage)] = storage.copy()
    return cases.Case(case.name, [(copies[id(s)], v) for s, v in case.boxes], case.reaches)


def _n_cells(case):
    return sum(v.size for v in cases.case_views(case))


def _histogram(ctx, scene, transform, lo, hi, bins, counts=None):
    counts = scene.histogram(transform, float(lo), float(hi), bins, counts)
    ctx.synchronize()
    return counts.cpu().numpy().astype(np.uint64)


LAYOUTS = cases.layout_cases() + [cases.all_layouts_case()]
EDGES = cases.value_edge_scenes()


@pytest.fixture(scope="module")
def tall():
    return cases.tall_box(cases.TALL_TILES)[0]


@pytest.fixture(scope="module")
def many():
    return cases.many_boxes()


# ---- 1, 2: statistics ---------------------------------------------------------------------------

def _check_stats(O, ctx, case):
    scene = ctx.create_scene(_device_boxes(ctx.device, case), ScalarTransform())
    got = scene.scalar_stats()
    want = O.scalar_stats(_oracle_boxes(O, case))
    plain = cases.numpy_stats(cases.case_views(case))
    assert want == plain, (want, plain)
    assert got == want, (case.name, got, want)
    return got


@pytest.mark.parametrize("case", LAYOUTS, ids=[c.name for c in LAYOUTS])
def test_statistics_of_every_layout(O, ctx, case):
    lo, hi, lo_pos, count = _check_stats(O, ctx, case)
    assert -1e4 < lo < 0.0 < lo_pos <= hi < 1e4 and 0 < count <= _n_cells(case)


def test_statistics_when_the_scans_loop(O, ctx, tall):
    """4102 tiles on 2048 workgroups: two and three trips of scalar_stats_kernel's loop, eight of
    reduce_stats_kernel's, the extremes in tiles that only later trips reach."""
    got = _check_stats(O, ctx, tall)
    assert got == (cases.TALL_MIN, cases.TALL_MAX, cases.TALL_MIN_POSITIVE, _n_cells(tall) - 1)


def test_statistics_of_many_boxes(O, ctx, many):
    got = _check_stats(O, ctx, many)
    assert got == (-1000.0, 1000.0, 1e-3, 30 * len(many.boxes))


@pytest.mark.parametrize("case", EDGES, ids=[c.name for c in EDGES])
def test_statistics_at_value_edges(O, ctx, case):
    got = _check_stats(O, ctx, case)
    if case.name in ("no_finite_cell", "empty"):
        assert got == NOTHING
    elif case.name == "no_positive_cell":
        assert got[1] == 0.0 and got[2] == INF and got[3] == _n_cells(case)
    elif case.name == "subnormal_min_positive":
        assert got[2] == 5e-324 and got[2] > 0.0
    elif case.name == "huge":
        assert got[:2] == (-1.7e308, 1.7e308)
    else:
        assert got == (2.0, 2.0, 2.0, 128 ** 3)


# ---- 3: histogram, every layout -----------------------------------------------------------------

# (log scale, normalise, bins): <LDS, SIMPLE>, <global, SIMPLE>, <LDS, general> and <global,
# general> without and with the logarithm
CONFIGS = [(False, True, 256), (False, True, 5000), (False, False, 64), (False, False, 4097),
           (True, True, 64), (True, True, 4097)]


def _three_ranges(scalar_range):
    lo, hi = np.float32(scalar_range[0]), np.float32(scalar_range[1])
    width = hi - lo
    quarter = width / np.float32(4)
    return [(lo, hi), (lo + quarter, hi - quarter), (hi + width, hi + width + width)]


@pytest.mark.parametrize("case", LAYOUTS, ids=[c.name for c in LAYOUTS])
def test_histogram_of_every_layout(O, ctx, case):
    stats = O.scalar_stats(_oracle_boxes(O, case))
    shared = ctx.create_scene(_device_boxes(ctx.device, case), ScalarTransform())
    n_cells = _n_cells(case)
    for log_scale, normalize, bins in CONFIGS:
        status, o_transform, _, _, _, o_range = O.scene_transform(stats[:3], stats[3], log_scale,
                                                                  normalize)
        assert status == 0
        transform, _, scalar_range = runtime.scene_transform_from_stats(stats[:3], stats[3],
                                                                        log_scale, normalize)
        assert scalar_range == o_range
        assert (scalar_range == (0.0, 1.0)) == normalize
        if not normalize:   # the data's own range, cast as the API casts it
            assert scalar_range == (float(np.float32(stats[0])), float(np.float32(stats[1])))
        for which, (lo, hi) in enumerate(_three_ranges(scalar_range)):
            at = (case.name, log_scale, normalize, bins, which)
            scene, safe = shared, case
            if log_scale:
                safe = _copy(case)
                cases.log_safe(cases.case_views(safe), o_transform, bins, lo, hi)
                assert O.scalar_stats(_oracle_boxes(O, safe)) == stats
                scene = ctx.create_scene(_device_boxes(ctx.device, safe), ScalarTransform())
            want = O.histogram(_oracle_boxes(O, safe), o_transform, lo, hi, bins)
            got = _histogram(ctx, scene, transform, lo, hi, bins)
            assert np.array_equal(got, want), (at, np.nonzero(got != want)[0][:8])
            assert int(got.sum()) == n_cells, at
            if which == 1 and n_cells >= 1000:      # both clamps of the range hold cells
                assert got[0] > want.sum() // bins and got[-1] > want.sum() // bins, at
            if which == 2:      # wholly above the data
                assert int(got[0]) == n_cells, at


def test_range_clamp_decides_the_bin_above_2_to_the_24_bins(O, ctx):
    """histogram_bin<SIMPLE> clamps the value to the range before it scales it.  For a cell above
    the range that is (max - min) * (1 / (max - min)) in float32, which may be 1 - 2^-24 where the
    value itself would scale to more than 1: with bins = 2^24 + 2 that product times the bin count
    rounds to 2^24, the last bin but one.  Below 2^24 bins both roads end in the last bin, so this
    is the one place where the clamp to the range shows."""
    case = cases.layout_cases()[1]
    bins = 2 ** 24 + 2
    lo = np.float32(0.25)
    hi = next(h for h in lo + np.float32(0.25) + np.arange(1, 200, dtype=np.float32) / np.float32(512)
              if (h - lo) * (np.float32(1) / (h - lo)) < np.float32(1))
    assert hi < 0.9 and np.float32((hi - lo) * (np.float32(1) / (hi - lo))) == np.float32(1 - 2.0 ** -24)
    boxes = _oracle_boxes(O, case)
    stats = O.scalar_stats(boxes)
    _, o_transform, *_ = O.scene_transform(stats[:3], stats[3], False, True)
    transform, _, _ = runtime.scene_transform_from_stats(stats[:3], stats[3], False, True)
    want = O.histogram(boxes, o_transform, lo, hi, bins)
    assert want[bins - 2] > 0 and want[bins - 1] == 0
    scene = ctx.create_scene(_device_boxes(ctx.device, case), ScalarTransform())
    got = _histogram(ctx, scene, transform, lo, hi, bins)
    assert got[bins - 2] == want[bins - 2] and got[bins - 1] == 0
    assert np.array_equal(got, want)


# ---- 4: cells on bin edges ----------------------------------------------------------------------

@pytest.mark.parametrize("bins", [256, 7, 4096, 4097])
def test_histogram_of_cells_on_bin_edges(O, ctx, bins):
    """The SIMPLE path clamps to [0, 1] after the cast to float32, the reference before it: the
    same bins for cells at, and one float64 and one float32 step either side of, every edge."""
    case, answer = cases.bin_edge_battery(bins)
    boxes = _oracle_boxes(O, case)
    stats = _check_stats(O, ctx, case)
    assert stats[:2] == (0.0, 1.0)
    status, o_transform, *_ = O.scene_transform(stats[:3], stats[3], False, True)
    transform, _, scalar_range = runtime.scene_transform_from_stats(stats[:3], stats[3], False, True)
    assert status == 0 and scalar_range == (0.0, 1.0)
    assert transform.normalization_min == 0.0 and transform.inverse_normalization_span == 1.0
    scene = ctx.create_scene(_device_boxes(ctx.device, case), ScalarTransform())
    got = _histogram(ctx, scene, transform, 0.0, 1.0, bins)
    want = O.histogram(boxes, o_transform, 0.0, 1.0, bins)
    assert np.array_equal(want, answer)
    assert np.array_equal(got, answer), np.nonzero(got != answer)[0][:8]


# ---- 5: tile counts -----------------------------------------------------------------------------

def _check_histograms(O, ctx, case):
    boxes = _oracle_boxes(O, case)
    stats = O.scalar_stats(boxes)
    scene = ctx.create_scene(_device_boxes(ctx.device, case), ScalarTransform())
    out = {}
    for normalize, bins in [(True, 256), (True, 4097), (False, 64), (False, 4097)]:
        _, o_transform, _, _, _, (lo, hi) = O.scene_transform(stats[:3], stats[3], False, normalize)
        transform, _, scalar_range = runtime.scene_transform_from_stats(stats[:3], stats[3], False,
                                                                        normalize)
        assert scalar_range == (lo, hi)
        want = O.histogram(boxes, o_transform, lo, hi, bins)
        got = _histogram(ctx, scene, transform, lo, hi, bins)
        assert np.array_equal(got, want), (case.name, normalize, bins)
        assert int(got.sum()) == _n_cells(case)
        out[normalize, bins] = (scene, transform, lo, hi, got)
    return out


@pytest.mark.parametrize("n_tiles", [1, 15, 16, 17])
def test_histogram_around_the_tiles_of_one_workgroup(O, ctx, n_tiles):
    _check_histograms(O, ctx, cases.tall_box(n_tiles)[0])


def test_histogram_of_many_tiles_and_twice_into_one_buffer(O, ctx, tall):
    scene, transform, lo, hi, once = _check_histograms(O, ctx, tall)[True, 4097]
    counts = scene.histogram(transform, lo, hi, 4097)
    twice = _histogram(ctx, scene, transform, lo, hi, 4097, counts)
    assert np.array_equal(twice, 2 * once)      # `once` equals the oracle's counts


def test_histogram_of_many_boxes(O, ctx, many):
    _check_histograms(O, ctx, many)


@pytest.mark.parametrize("bins", [16, 4097])
def test_histogram_of_a_constant_field(O, ctx, bins):
    case = EDGES[4]
    assert case.name == "constant"
    boxes = _oracle_boxes(O, case)
    stats = (2.0, 2.0, 2.0, 128 ** 3)
    _, o_transform, *_ = O.scene_transform(stats[:3], stats[3], False, True)
    transform, _, _ = runtime.scene_transform_from_stats(stats[:3], stats[3], False, True)
    scene = ctx.create_scene(_device_boxes(ctx.device, case), ScalarTransform())
    got = _histogram(ctx, scene, transform, 0.0, 1.0, bins)
    assert np.array_equal(got, O.histogram(boxes, o_transform, 0.0, 1.0, bins))
    assert got[0] == 2_097_152 and not got[1:].any()


def test_histogram_of_no_boxes_and_of_no_finite_cell(O, ctx):
    transform = ScalarTransform(normalize_to_unit_range=True)
    o_transform = O.make_transform()
    empty = ctx.create_scene([], ScalarTransform())
    assert not _histogram(ctx, empty, transform, 0.0, 1.0, 64).any()
    case = EDGES[0]
    assert case.name == "no_finite_cell"
    scene = ctx.create_scene(_device_boxes(ctx.device, case), ScalarTransform())
    got = _histogram(ctx, scene, transform, 0.0, 1.0, 64)     # every such cell counts as 0.0
    assert np.array_equal(got, O.histogram(_oracle_boxes(O, case), o_transform, 0.0, 1.0, 64))
    assert got[0] == _n_cells(case)


# ---- 6: ranks -----------------------------------------------------------------------------------

RANK_BINS = 128


def _transform_fields(t):
    return np.array([float(t.log_scale_input), float(t.normalize_to_unit_range), t.positive_floor,
                     t.normalization_min, t.inverse_normalization_span], dtype=np.float64)


def _geometry_and_histogram(ctx, meta, local, group=None, world=1):
    out = {}
    for log_scale in (False, True):
        geometry = api.build_scene_geometry(ctx, meta, local, VolumeBounds(), log_scale, True,
                                            group, world)
        out[f"transform_{int(log_scale)}"] = _transform_fields(geometry.scalar_transform)
        out[f"ranges_{int(log_scale)}"] = np.array(
            list(geometry.scalar_range) + list(geometry.processed_scalar_range), dtype=np.float64)
    result = api.compute_scene_histogram(ctx, meta, local, False, RANK_BINS, group, world)
    out["counts"] = result["counts"]
    out["samples"] = np.array([result["samples"]])
    out["original_range"] = np.array(result["original_range"], dtype=np.float64)
    return out


def _metadata(case):
    return [AmrBox(CORNERS[0], CORNERS[1], dims=v.shape[::-1]) for v in cases.case_views(case)]


def _stats_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        ctx = runtime.Context(0)
        case = cases.all_layouts_case()
        # dealt round-robin to ranks 0 and 1: a third rank holds no box at all
        mine = cases.Case(case.name, [b for i, b in enumerate(case.boxes) if i % 2 == rank],
                          case.reaches)
        assert len(mine.boxes) == (5, 4, 0)[rank]
        out = _geometry_and_histogram(ctx, _metadata(case), _device_boxes(ctx.device, mine),
                                      dist.group.WORLD, world)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_on_one_gpu_equal_the_one_rank_answer(O, ctx, tmp_path, world):
    """The MIN / MAX / SUM reductions of build_scene_geometry and compute_scene_histogram, staged
    through the host on a gloo group; in the world of three, rank 2 has no boxes."""
    spawn_ranks(_stats_worker, world, lambda port: (world, port, str(tmp_path)))
    case = cases.all_layouts_case()
    one = _geometry_and_histogram(ctx, _metadata(case), _device_boxes(ctx.device, case))
    boxes = _oracle_boxes(O, case)
    stats = O.scalar_stats(boxes)
    for log_scale in (False, True):
        status, o_transform, _, _, o_processed, o_range = O.scene_transform(
            stats[:3], stats[3], log_scale, True)
        assert status == 0
        assert np.array_equal(one[f"transform_{int(log_scale)}"], _transform_fields(o_transform))
        assert np.array_equal(one[f"ranges_{int(log_scale)}"],
                              np.array(list(o_range) + list(o_processed), dtype=np.float64))
    _, o_transform, *_ = O.scene_transform(stats[:3], stats[3], False, True)
    assert np.array_equal(one["counts"], O.histogram(boxes, o_transform, 0.0, 1.0, RANK_BINS))
    assert one["samples"][0] == _n_cells(case)
    assert np.array_equal(one["original_range"],
                          np.array([np.float32(stats[0]), np.float32(stats[1])], dtype=np.float64))
    for rank in range(world):
        got = np.load(tmp_path / f"rank{rank}.npz")
        assert sorted(got.files) == sorted(one)
        for key, want in one.items():
            assert got[key].dtype == want.dtype and np.array_equal(got[key], want), (rank, key)
