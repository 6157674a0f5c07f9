"""The inputs of test_scene_stats_gpu.py held to what they claim, without a GPU: the layouts'
parities, the tile numbers of the placed extremes, the poison around the views, and the oracle's
statistics and histogram against plain numpy answers."""
import numpy as np
import pytest

import scene_stats_cases as cases

INF = float("inf")
NOTHING = (INF, -INF, INF, 0)


def _oracle_boxes(O, case):
    return [O.make_box(v, (0, 0, 0), (1, 1, 1)) for v in cases.case_views(case)]


def _storages(case):
    seen = {}
    for storage, _ in case.boxes:
        seen[id(storage)] = storage
    return list(seen.values())


def _stats_everywhere(O, case):
    """The oracle's statistics over every element of the case's storages."""
    return O.scalar_stats([O.make_box(cases.storage_as_view(s), (0, 0, 0), (1, 1, 1))
                           for s in _storages(case)])


def _carries_all_poisons(cells):
    cells = np.asarray(cells).reshape(-1)
    return (np.isnan(cells).any() and
            all((cells == p).any() for p in cases.POISON[:3]))


LAYOUT_CASES = cases.layout_cases()


@pytest.mark.parametrize("row,case", list(zip(cases.LAYOUTS, LAYOUT_CASES)),
                         ids=[c.name for c in LAYOUT_CASES])
def test_layout_is_what_the_table_says(row, case):
    name, offset_parity, j_parity, k_parity, nx, ny, nz, reaches = row
    (storage, (offset, shape, strides)), = case.boxes
    assert case.name == name and case.reaches == reaches
    assert shape == (nz, ny, nx) and strides[2] == 1
    assert ny in (1, 3, 5, 9) and nz in (1, 3, 5, 9)
    assert offset % 2 == offset_parity and strides[1] % 2 == j_parity
    assert k_parity is None or strides[0] % 2 == k_parity
    assert cases.is_paired(offset, strides[1], strides[0]) == name.startswith("pair_")
    view = cases.host_view(storage, case.boxes[0][1])
    assert view.shape == shape and view.strides == tuple(8 * s for s in strides)
    assert view.ctypes.data == storage.ctypes.data + 8 * offset
    # two cells of poison on every side of every row, two rows and two planes around the box
    kstride, jstride, _ = strides
    assert jstride >= nx + 4 and kstride >= (ny + 4) * jstride
    assert offset >= 2 * kstride + 2 * jstride + 2
    assert offset + (nz + 1) * kstride + (ny + 1) * jstride + nx + 2 <= storage.size
    inside = np.zeros(storage.size, bool)
    for k in range(nz):
        for j in range(ny):
            at = offset + k * kstride + j * jstride
            inside[at:at + nx] = True
            assert _carries_all_poisons(storage[[at - 2, at - 1, at + nx, at + nx + 1]])
        for j in (-2, -1, ny, ny + 1):      # the rows before and after the plane's rows
            at = offset + k * kstride + j * jstride
            assert _carries_all_poisons(storage[at - 2:at + nx + 2])
    for k in (-2, -1, nz, nz + 1):          # the planes before and after the box
        for j in range(ny):
            at = offset + k * kstride + j * jstride
            assert _carries_all_poisons(storage[at - 2:at + nx + 2])
    assert inside.sum() == nx * ny * nz
    outside = storage[~inside]
    assert (np.isnan(outside) | np.isin(outside, cases.POISON[:3])).all()
    cells = storage[inside]
    bad = ~np.isfinite(cells)
    assert np.abs(cells[~bad]).max() < 1e4
    if cells.size > 1000:
        assert 0.005 < bad.mean() < 0.05
    elif name != "pair_one_cell_rows":
        assert bad.any() or cells.size < 50


def test_layouts_reach_both_load_paths_and_the_tail():
    paired = {c.name: cases.is_paired(c.boxes[0][1][0], c.boxes[0][1][2][1], c.boxes[0][1][2][0])
              for c in LAYOUT_CASES}
    assert sum(paired.values()) == 6 and len(paired) == 9
    odd_nx_paired = [c.name for c in LAYOUT_CASES if paired[c.name] and c.boxes[0][1][1][2] % 2]
    assert set(odd_nx_paired) == {"pair_odd_tail", "pair_chunk_on_last_cell", "pair_one_cell_rows",
                                  "pair_127"}
    assert [c.boxes[0] for c in LAYOUT_CASES][3][1][1][2] == 1
    assert cases.scene_tiles(cases.all_layouts_case()) == sum(cases.scene_tiles(c) for c in LAYOUT_CASES)


ALL_STATS_CASES = (LAYOUT_CASES + [cases.all_layouts_case(), cases.tall_box(cases.TALL_TILES)[0],
                                   cases.many_boxes()] + cases.value_edge_scenes())


@pytest.mark.parametrize("case", ALL_STATS_CASES, ids=[c.name for c in ALL_STATS_CASES])
def test_oracle_statistics_equal_numpy(O, case):
    views = cases.case_views(case)
    want = cases.numpy_stats(views)
    got = O.scalar_stats(_oracle_boxes(O, case))
    assert got == want, (got, want)
    assert want[3] <= sum(v.size for v in views)


POISONED = LAYOUT_CASES + [cases.all_layouts_case(), cases.many_boxes()]


@pytest.mark.parametrize("case", POISONED, ids=[c.name for c in POISONED])
def test_a_read_outside_a_view_would_show(O, case):
    """Every statistic over the whole storages differs from the views' own."""
    want = cases.numpy_stats(cases.case_views(case))
    everywhere = _stats_everywhere(O, case)
    assert everywhere[0] == -1e308 and everywhere[1] == 1e308 and everywhere[2] == 5e-324
    assert all(e != w for e, w in zip(everywhere, want)), (everywhere, want)
    assert np.isnan(np.concatenate(_storages(case))).sum() > \
        sum(int(np.isnan(v).sum()) for v in cases.case_views(case))


def test_python_tiles_count_and_decode():
    for nx, ny, nz in [(3, 5, 8), (131, 9, 5), (129, 5, 1), (256, 3, 5), (1, 9, 9), (300, 7, 12)]:
        n = cases.cell_tiles(nx, ny, nz)
        seen = np.zeros((nz, ny, nx), np.int64)
        for t in range(n):
            sl = cases.tile_slices((nz, ny, nx), t)
            assert all(s.start < s.stop for s in sl)
            seen[sl] += 1
            k, j, i = (s.start for s in sl)
            assert cases.tile_of_cell(nx, ny, i, j, k) == t
        assert (seen == 1).all()
    assert cases.cell_tile_of(300, 7, 0) == (0, 0, 0)
    assert cases.cell_tile_of(300, 7, 1) == (1, 0, 0)       # the chunk runs fastest
    assert cases.cell_tile_of(300, 7, 3) == (0, 1, 0)       # then the brick along y
    assert cases.cell_tile_of(300, 7, 6) == (0, 0, 1)       # then along z


@pytest.mark.parametrize("n_tiles", [1, 15, 16, 17, cases.TALL_TILES])
def test_tall_box_has_its_tiles(n_tiles):
    case, placed = cases.tall_box(n_tiles)
    (cells, view), = case.boxes
    nz, ny, nx = cells.shape
    assert view is None and cells.flags.c_contiguous
    assert cases.cell_tiles(nx, ny, nz) == n_tiles == cases.scene_tiles(case)
    assert nx == 3 and ny == (5 if n_tiles % 2 == 0 else 3)
    k, j, i = placed["nan"]
    assert cases.tile_of_cell(nx, ny, i, j, k) == n_tiles - 1
    assert np.isnan(cells[placed["nan"]]) and (~np.isfinite(cells)).sum() == 1


def test_tall_box_extremes_are_where_the_loops_need_them():
    assert cases.TALL_TILES == 2 * cases.SCAN_WORKGROUPS + 6 == 4102
    case, placed = cases.tall_box(cases.TALL_TILES)
    cells = case.boxes[0][0]
    nz, ny, nx = cells.shape
    lo, hi, lo_pos, count = cases.numpy_stats([cells])
    assert (lo, hi, lo_pos) == (cases.TALL_MIN, cases.TALL_MAX, cases.TALL_MIN_POSITIVE)
    assert count == cells.size - 1
    tiles = {}
    for what, value in (("min", lo), ("max", hi), ("min_positive", lo_pos)):
        where = np.argwhere(cells == value)
        assert where.shape == (1, 3) and tuple(where[0]) == placed[what]      # unique
        k, j, i = where[0]
        tiles[what] = cases.tile_of_cell(nx, ny, i, j, k)
    groups = cases.SCAN_WORKGROUPS
    assert tiles["min"] >= 2 * groups                        # a third trip
    assert groups <= tiles["max"] < 2 * groups               # a second trip
    assert tiles["min_positive"] < groups                    # a first trip
    assert tiles["max"] % groups >= 256 and tiles["min_positive"] % groups >= 256
    last = cases.tile_slices(cells.shape, tiles["min_positive"])
    assert placed["min_positive"] == tuple(s.stop - 1 for s in last)
    # everything else lies strictly inside the extremes
    rest = cells[np.isfinite(cells)]
    rest = rest[~np.isin(rest, [lo, hi, lo_pos])]
    assert rest.size == cells.size - 4
    assert rest.min() > lo and rest.max() < hi and rest[rest > 0].min() > lo_pos


def test_many_boxes_layout_and_extremes():
    n = 1500
    case = cases.many_boxes(n)
    assert len(case.boxes) == n and cases.scene_tiles(case) == 2 * n
    views = cases.case_views(case)
    storage = case.boxes[0][0]
    offsets = [view[0] for _, view in case.boxes]
    assert all(s is storage for s, _ in case.boxes)
    assert all(b - a == 35 for a, b in zip(offsets, offsets[1:]))
    assert [o % 2 for o in offsets[:4]] == [0, 1, 0, 1]
    for _, (offset, shape, strides) in case.boxes:
        assert shape == (5, 3, 2) and strides == (6, 2, 1)
        assert cases.cell_tiles(2, 3, 5) == 2
        assert _carries_all_poisons(storage[offset - 4:offset])
        assert _carries_all_poisons(storage[offset + 30:offset + 34])
    lo, hi, lo_pos, count = cases.numpy_stats(views)
    assert count == 30 * n
    for value, box in ((lo, n - 1), (hi, 1), (lo_pos, n // 2)):
        holders = [b for b, v in enumerate(views) if (v == value).any()]
        assert holders == [box] and (views[box] == value).sum() == 1


def test_value_edge_scenes(O):
    scenes = {c.name: c for c in cases.value_edge_scenes()}
    assert list(scenes) == ["no_finite_cell", "no_positive_cell", "subnormal_min_positive", "huge",
                            "constant", "empty"]
    for name, case in scenes.items():
        for cells, view in case.boxes:
            assert view is None and cells.flags.c_contiguous
            assert cells.shape == ((128, 128, 128) if name == "constant" else cases.EDGE_SHAPE)
    stats = {name: O.scalar_stats(_oracle_boxes(O, c)) for name, c in scenes.items()}
    for name in ("no_finite_cell", "empty"):
        assert stats[name] == NOTHING
        for log_scale in (False, True):
            status = O.scene_transform(stats[name][:3], stats[name][3], log_scale, True)[0]
            assert status == (1 if log_scale else 2)
        assert O.scene_transform(stats[name][:3], 0, False, False)[0] == 2
    assert scenes["empty"].boxes == []
    cells = scenes["no_finite_cell"].boxes[0][0]
    assert all(f(cells).any() for f in (np.isnan, np.isposinf, np.isneginf))
    lo, hi, lo_pos, count = stats["no_positive_cell"]
    cells = scenes["no_positive_cell"].boxes[0][0]
    assert lo < 0.0 and hi == 0.0 and lo_pos == INF and count == cells.size
    zeros = cells[cells == 0.0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()
    assert O.scene_transform((lo, hi, lo_pos), count, True, True)[0] == 1
    lo, hi, lo_pos, count = stats["subnormal_min_positive"]
    cells = scenes["subnormal_min_positive"].boxes[0][0]
    assert lo_pos == 5e-324 and 0.0 < lo_pos < np.finfo(np.float64).tiny
    positive = np.unique(cells[cells > 0.0])
    assert positive[0] == 5e-324 and positive[1] == 2.3e-308 >= np.finfo(np.float64).tiny
    assert (cells == 5e-324).sum() == 1
    assert stats["huge"][:2] == (-1.7e308, 1.7e308)
    assert stats["constant"] == (2.0, 2.0, 2.0, 128 ** 3)


@pytest.mark.parametrize("bins", [256, 7, 4096, 4097])
def test_bin_edge_battery_known_answer(O, bins):
    case, answer = cases.bin_edge_battery(bins)
    cells = case.boxes[0][0]
    assert cells.shape[:2] == (4, 4) and cells.min() == 0.0 and cells.max() == 1.0
    edges = np.arange(bins + 1) / bins
    assert np.isin(edges, cells).all()
    assert np.isin(np.nextafter(edges[1:], 0.0), cells).all()
    assert np.isin(np.nextafter(edges[:-1], 1.0), cells).all()
    assert np.isin(edges.astype(np.float32).astype(np.float64), cells).all()
    boxes = _oracle_boxes(O, case)
    stats = O.scalar_stats(boxes)
    status, transform, _, _, _, scalar_range = O.scene_transform(stats[:3], stats[3], False, True)
    assert status == 0 and scalar_range == (0.0, 1.0)
    assert transform.normalization_min == 0.0 and transform.inverse_normalization_span == 1.0
    got = O.histogram(boxes, transform, 0.0, 1.0, bins)
    assert np.array_equal(got, answer)
    assert int(answer.sum()) == cells.size
    # the vectorised answer against min(int(float32(v) * float32(bins)), bins - 1) cell by cell
    slow = np.zeros(bins, np.uint64)
    for v in cells.reshape(-1)[::97]:
        slow[min(int(np.float32(v) * np.float32(bins)), bins - 1)] += 1
    index = (cells.reshape(-1)[::97].astype(np.float32) * np.float32(bins)).astype(np.int64)
    assert np.array_equal(slow, np.bincount(np.minimum(index, bins - 1), minlength=bins))


@pytest.mark.parametrize("bins", [64, 4097])
def test_log_safe_keeps_its_cap(O, bins):
    cells = np.exp(np.random.default_rng(cases.SEED).normal(0.0, 2.0, (8, 16, 256)))
    most = cells.size // 100
    box = [O.make_box(cells, (0, 0, 0), (1, 1, 1))]
    stats = O.scalar_stats(box)
    status, transform, *_ = O.scene_transform(stats[:3], stats[3], True, True)
    assert status == 0
    replaced = cases.log_safe([cells], transform, bins)
    assert replaced <= most                          # 1 %; about bins * 2^-21 of 32,768 cells go
    assert replaced > 0 or bins == 64
    assert O.scalar_stats(box) == stats              # the extremes stay
    assert cases.log_safe([cells], transform, bins) == 0
    # a narrower range widens the margin with its inverse width
    assert cases.log_safe([cells], transform, bins, 0.25, 0.75) <= 2 * most
    assert cases.log_safe([cells], transform, bins, 0.25, 0.75) == 0
    assert O.scalar_stats(box) == stats


def test_log_safe_refuses_to_gut_a_field(O):
    cells = np.full((4, 4, 16), np.e)
    cells[0, 0, 0], cells[0, 0, 1] = 1.0, np.e ** 2     # x = bins / 2 for all the others
    transform = O.make_transform(True, True, 1.0, 0.0, 0.5)
    with pytest.raises(AssertionError):
        cases.log_safe([cells], transform, 64)
