"""Inputs of the scene statistics / histogram tests (avr_scene_stats.hip), numpy only: layouts
that take each load path of for_each_cell, shapes that make the scans loop, value edges, and cells
on bin edges.  test_scene_stats_cases.py holds the builders to their claims on the CPU;
test_scene_stats_gpu.py runs the kernels on them.

A box is (storage, view).  view None: the storage is the box, a C-contiguous [nz, ny, nx] array.
Otherwise the storage is one flat float64 array and view = (offset, (nz, ny, nx), (kstride,
jstride, 1)) in elements -- the slicing of a dense 3-D array cannot have an odd k stride over an
even j stride, which plotfile boxes do have and the layout table asks for.  host_view() takes the
view with numpy, the GPU tests take the same one with torch.as_strided on the uploaded storage."""
from collections import namedtuple

import numpy as np

SEED = 4242
# what a read outside a view would bring in: each of the first three moves one of min, max and min
# positive and all three move the finite count; NaN moves the cell count of a histogram
POISON = np.array([1e308, -1e308, 5e-324, np.nan])
BRICK = 4            # kBrickY = kBrickZ
CHUNK = 128          # kClassifyChunk
SCAN_WORKGROUPS = 2048   # kScanWorkgroups

Case = namedtuple("Case", "name boxes reaches")


def host_view(storage, view):
    if view is None:
        return storage
    offset, shape, strides = view
    return np.lib.stride_tricks.as_strided(storage[offset:], shape, tuple(8 * s for s in strides))


def case_views(case):
    return [host_view(storage, view) for storage, view in case.boxes]


# ---- avr_cell_tiles.h in Python -------------------------------------------------------------------

def cell_tiles(nx, ny, nz):
    """Tiles of one box: 128-cell chunks along x times 4-row bricks along y times 4-plane bricks
    along z."""
    return (-(-nx // CHUNK)) * (-(-ny // BRICK)) * (-(-nz // BRICK))


def cell_tile_of(nx, ny, local):
    """(chunk, bj, bk) of tile `local`: the chunk runs fastest, then the brick along y, then z."""
    chunks, bricks_y = -(-nx // CHUNK), -(-ny // BRICK)
    chunk = local % chunks
    local //= chunks
    return chunk, local % bricks_y, local // bricks_y


def tile_of_cell(nx, ny, i, j, k):
    chunks, bricks_y = -(-nx // CHUNK), -(-ny // BRICK)
    return i // CHUNK + chunks * (j // BRICK + bricks_y * (k // BRICK))


def tile_slices(shape, local):
    """The cells [k, j, i] of tile `local` of a box of this [nz, ny, nx] shape, as slices."""
    nz, ny, nx = shape
    chunk, bj, bk = cell_tile_of(nx, ny, local)
    return (slice(BRICK * bk, min(BRICK * bk + BRICK, nz)),
            slice(BRICK * bj, min(BRICK * bj + BRICK, ny)),
            slice(CHUNK * chunk, min(CHUNK * chunk + CHUNK, nx)))


def scene_tiles(case):
    return sum(cell_tiles(*v.shape[::-1]) for v in case_views(case))


# ---- the plain answers ----------------------------------------------------------------------------

def numpy_stats(views):
    """(min, max, min positive, finite count) in float64 numpy."""
    lo, hi, lo_pos, count = np.inf, -np.inf, np.inf, 0
    for v in views:
        cells = np.asarray(v, dtype=np.float64).reshape(-1)
        cells = cells[np.isfinite(cells)]
        if cells.size:
            lo, hi = min(lo, float(cells.min())), max(hi, float(cells.max()))
            count += int(cells.size)
            if (cells > 0).any():
                lo_pos = min(lo_pos, float(cells[cells > 0].min()))
    return lo, hi, lo_pos, count


def storage_as_view(storage):
    """Every element of a storage as one row of cells: what a scan without bounds would see."""
    return storage.reshape(1, 1, -1)


# ---- layouts --------------------------------------------------------------------------------------

# name, offset parity, jstride parity, kstride parity (None: any), nx, ny, nz, reaches
LAYOUTS = [
    ("pair_even", 0, 0, 0, 256, 3, 5, "pairs, whole chunks"),
    ("pair_odd_tail", 0, 0, 0, 131, 9, 5, "pairs + single last cell"),
    ("pair_chunk_on_last_cell", 0, 0, 0, 129, 5, 1, "2nd chunk = one single cell"),
    ("pair_one_cell_rows", 0, 0, 0, 1, 9, 9, "pair path, i + 1 < nx false at once"),
    ("pair_two", 0, 0, 0, 2, 5, 3, "one pair per row"),
    ("pair_127", 0, 0, 0, 127, 1, 9, "last lane's pair cut"),
    ("unaligned", 1, 0, 0, 131, 3, 9, "single cells, base 8 mod 16"),
    ("odd_jstride", 0, 1, None, 130, 5, 3, "single cells"),
    ("odd_kstride", 0, 0, 1, 130, 3, 5, "single cells"),
]


def is_paired(offset, jstride, kstride):
    """for_each_cell's `paired`, for a storage that starts on a 16-byte boundary."""
    return offset % 2 == 0 and jstride % 2 == 0 and kstride % 2 == 0


def _poisoned_storage(size):
    return POISON[np.arange(size) % 4].copy()


def _poison_row_ends(storage, offset, shape, strides):
    """The two cells left and the two right of every row of the view carry all four poisons, in
    an order that turns with the row."""
    nz, ny, nx = shape
    for k in range(nz):
        for j in range(ny):
            row = offset + k * strides[0] + j * strides[1]
            turn = np.roll(POISON, j + k)
            storage[[row - 2, row - 1, row + nx, row + nx + 1]] = turn


def _field_cells(rng, shape):
    """normal(1, 2) * 100 with about 2 % of NaN / +Inf / -Inf."""
    cells = rng.normal(1.0, 2.0, shape) * 100.0
    flat = cells.reshape(-1)
    bad = rng.random(flat.size) < 0.02
    flat[bad] = rng.choice([np.nan, np.inf, -np.inf], size=int(bad.sum()))
    return cells


def _layout_box(rng, offset_parity, j_parity, k_parity, nx, ny, nz):
    jstride = nx + 4
    jstride += (jstride % 2) != j_parity
    kstride = (ny + 4) * jstride
    if k_parity is not None:
        kstride += (kstride % 2) != k_parity
    offset = 2 * kstride + 2 * jstride + 2     # two planes, two rows and two cells of poison before
    offset += (offset % 2) != offset_parity
    storage = _poisoned_storage(offset + (nz + 2) * kstride)
    shape, strides = (nz, ny, nx), (kstride, jstride, 1)
    _poison_row_ends(storage, offset, shape, strides)
    view = (offset, shape, strides)
    host_view(storage, view)[...] = _field_cells(rng, shape)
    return storage, view


def layout_cases():
    """One scene of one box per row of LAYOUTS: a view into a storage of poison."""
    rng = np.random.default_rng(SEED)
    return [Case(name, [_layout_box(rng, op, jp, kp, nx, ny, nz)], reaches)
            for name, op, jp, kp, nx, ny, nz, reaches in LAYOUTS]


def all_layouts_case():
    """The nine layouts as one scene of nine boxes."""
    return Case("all_layouts", [c.boxes[0] for c in layout_cases()], "every load path in one scene")


# ---- scans that loop ------------------------------------------------------------------------------

TALL_TILES = 2 * SCAN_WORKGROUPS + 6
# tile numbers of the extremes of tall_box(TALL_TILES): the minimum on a third trip of its
# workgroup, the maximum on a second trip, the min positive on a first, the latter two in
# workgroups whose partial results the final reduction reaches on a later trip of its own loop
TALL_MIN_TILE, TALL_MAX_TILE, TALL_MIN_POSITIVE_TILE = 4099, 2048 + 1000, 1501
TALL_MIN, TALL_MAX, TALL_MIN_POSITIVE = -1000.0, 1000.0, 1e-3


def _last_cell(slices):
    return tuple(s.stop - 1 for s in slices)


def tall_box(n_tiles):
    """One contiguous box with exactly n_tiles tiles: 3 x 5 x 2 n_tiles cells (two bricks along y)
    for an even count, 3 x 3 x 4 n_tiles (one brick along y) for an odd one.  Cells: +-[10, 100],
    strictly inside the extremes, which are placed as TALL_* say where the box has those tiles;
    one cell of the last tile is NaN."""
    rng = np.random.default_rng(SEED + n_tiles)
    shape = (2 * n_tiles, 5, 3) if n_tiles % 2 == 0 else (4 * n_tiles, 3, 3)
    cells = rng.uniform(10.0, 100.0, shape) * rng.choice([-1.0, 1.0], shape)
    placed = {}
    if n_tiles > TALL_MIN_TILE:
        for what, tile, value in (("min", TALL_MIN_TILE, TALL_MIN), ("max", TALL_MAX_TILE, TALL_MAX)):
            k, j, i = (s.start for s in tile_slices(shape, tile))
            placed[what] = (k + 1, j, i + 1)
            cells[placed[what]] = value
        placed["min_positive"] = _last_cell(tile_slices(shape, TALL_MIN_POSITIVE_TILE))
        cells[placed["min_positive"]] = TALL_MIN_POSITIVE
    k, j, i = (s.start for s in tile_slices(shape, n_tiles - 1))
    placed["nan"] = (k, j, i + 2)
    cells[placed["nan"]] = np.nan
    return Case(f"tall_{n_tiles}", [(cells, None)], f"{n_tiles} tiles"), placed


def many_boxes(n=1500):
    """n boxes of 2 x 3 x 5 cells (two tiles each), dense views at alternately even and odd
    offsets into one storage, five cells of poison between neighbours.  The minimum is in the
    last box, the maximum in box 1, the min positive in box n // 2."""
    rng = np.random.default_rng(SEED + 1)
    shape, strides, pitch = (5, 3, 2), (6, 2, 1), 35
    storage = _poisoned_storage(4 + pitch * n)
    boxes = []
    for b in range(n):
        view = (4 + pitch * b, shape, strides)
        cells = rng.uniform(10.0, 100.0, shape) * rng.choice([-1.0, 1.0], shape)
        if b == n - 1:
            cells[4, 2, 1] = -1000.0
        if b == 1:
            cells[0, 0, 0] = 1000.0
        if b == n // 2:
            cells[2, 1, 1] = 1e-3
        host_view(storage, view)[...] = cells
        boxes.append((storage, view))
    return Case(f"many_boxes_{n}", boxes, f"{n} boxes, {2 * n} tiles")


# ---- value edges ----------------------------------------------------------------------------------

EDGE_SHAPE = (4, 4, 130)     # contiguous: even strides, the pair path, a second chunk of one pair


def value_edge_scenes():
    rng = np.random.default_rng(SEED + 2)
    n = int(np.prod(EDGE_SHAPE))

    def box(flat):
        return [(np.ascontiguousarray(flat, dtype=np.float64).reshape(EDGE_SHAPE), None)]

    nonfinite = rng.choice([np.nan, np.inf, -np.inf], size=n)
    no_positive = -rng.uniform(0.0, 50.0, n)
    no_positive[::3] = 0.0
    no_positive[1::7] = -0.0
    subnormal = rng.choice([-3.0, -0.0, 0.0, 1.0, 7.5], size=n)
    subnormal[n - 1] = 5e-324        # the odd last cell of the last row's second chunk
    subnormal[5] = 2.3e-308
    huge = rng.normal(0.0, 1e300, n)
    huge[130 + 129] = -1.7e308
    huge[77] = 1.7e308
    return [
        Case("no_finite_cell", box(nonfinite), "only NaN / +Inf / -Inf"),
        Case("no_positive_cell", box(no_positive), "negatives and both zeros: min positive stays +inf"),
        Case("subnormal_min_positive", box(subnormal), "min positive 5e-324, the next 2.3e-308"),
        Case("huge", box(huge), "min -1.7e308, max 1.7e308"),
        Case("constant", [(np.full((128, 128, 128), 2.0), None)], "one bin takes 2,097,152 cells"),
        Case("empty", [], "no boxes: a rank beyond the box count"),
    ]


# ---- cells on bin edges ---------------------------------------------------------------------------

def bin_edge_battery(bins):
    """(case, answer): a 4 x 4 x N field with min 0 and max 1 holding every edge k / bins, its
    float64 neighbours and the float32 neighbours of float32(k / bins), padded with 0.5; and the
    bin counts worked out in numpy float32."""
    e = np.arange(bins + 1, dtype=np.float64) / bins
    e32 = e.astype(np.float32)
    cells = np.concatenate([
        e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
        np.nextafter(e32, np.float32(-np.inf)).astype(np.float64),
        np.nextafter(e32, np.float32(np.inf)).astype(np.float64), e32.astype(np.float64)])
    cells = cells[(cells >= 0.0) & (cells <= 1.0)]
    assert cells.min() == 0.0 and cells.max() == 1.0
    n = -(-cells.size // 16)
    cells = np.concatenate([cells, np.full(16 * n - cells.size, 0.5)])
    index = (cells.astype(np.float32) * np.float32(bins)).astype(np.int64)
    answer = np.bincount(np.minimum(index, bins - 1), minlength=bins).astype(np.uint64)
    case = Case(f"bin_edges_{bins}", [(cells.reshape(4, 4, n), None)], "cells at and beside bin edges")
    return case, answer


# ---- log scale ------------------------------------------------------------------------------------

def log_safe(views, transform, bins, range_min=0.0, range_max=1.0):
    """Makes a log-scale histogram of `views` independent of the last bit of log(): the device's
    log and the C library's may differ there, which after the cast to float32 and the three
    float32 operations that follow can move a cell over a bin edge only if x = normalised * bins is
    within bins * 2^-22 (times the inverse range width where the range is narrower than one) of
    that edge.  x is worked out here in float64; every cell that close to an edge 1 .. bins - 1 is
    overwritten in place by the box's first cell that is not.  (0 and bins are no edges: the
    clamps hold cells there.)  At most 1 % of the cells may go.  Returns how many went."""
    floor = float(transform.positive_floor)
    range_min, range_max = float(np.float32(range_min)), float(np.float32(range_max))
    inverse_width = 1.0 / (range_max - range_min)
    margin = bins * 2.0 ** -22 * max(1.0, inverse_width)
    replaced = total = 0
    for view in views:
        v = np.where(np.isfinite(view), view, 0.0)
        v = np.log(np.where(v > floor, v, floor))
        if transform.normalize_to_unit_range:
            v = np.clip((v - transform.normalization_min) * transform.inverse_normalization_span,
                        0.0, 1.0)
        x = (v - range_min) * inverse_width * bins
        edge = np.clip(np.rint(x), 1, bins - 1)
        unsafe = np.abs(x - edge) <= margin
        if unsafe.any():
            view[unsafe] = view[~unsafe][0]
        replaced += int(unsafe.sum())
        total += view.size
    assert replaced * 100 <= total, (replaced, total)
    return replaced
