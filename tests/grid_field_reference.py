"""The reference of the grid fields ("Grid fields"): plain numpy on a plotfile's own
level arrays, as gradient_reference.leaf_arrays gives them (per level the origin, the leaf mask
and the values over the level's domain).  It never sees the scene's boxes.

grid [nz, ny, nx] holds the cells lo + (i, j, k) of level L.  The leaf with index I of level l,
per axis, with R the product of the ratios between l and L:
  l == L            G = I; grid[G - lo] with its bits kept if G lies in the region, else fill;
  l > L, constant   G = I // R (floors, also below zero), then as above;
  l > L, linear     p = I - G R, c = 2 p + 1 - R, t = f64(|c|) / f64(2 R), N = G - 1 for c < 0 and
                    G + 1 otherwise; an N outside the region wraps into it (periodic) or becomes G;
                    fill if G is outside on any axis, else the eight values combined along x, then
                    y, then z, each step a + t * (b - a);
  l < L             s = +0.0, n = 0; for kk, then jj, then ii ascending in [0, R) the grid cell
                    I R + (ii, jj, kk), if it lies in the region, gives s = s + v and n += 1; with
                    n > 0 the value is s / f64(n), else fill.
outside counts the leaves that got fill, partial those with l < L and 0 < n < R^3.
Vectorised over the leaves of a level; the loops over kk, jj, ii keep the order of the additions.
"""
import numpy as np

from gradient_reference import leaf_arrays


def _factor(ref_ratio, a, b):
    lo, hi = min(a, b), max(a, b)
    return int(np.prod([int(r) for r in ref_ratio[lo:hi]], dtype=np.int64)) if hi > lo else 1


def _bits(value):
    return np.array([value], dtype=np.float64).view(np.uint64)[0]


def grid_cells(grid, level, lo, cell_level, index, ref_ratio, interpolation=0, periodic=False,
               fill=np.nan):
    """The rules for the level-`cell_level` indices index [3, n] (i, j, k) -> (values [n],
    got fill [n], partial [n])."""
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    nz, ny, nx = grid.shape
    dims = np.array([nx, ny, nz], dtype=np.int64)[:, None]
    first = np.array([int(v) for v in lo], dtype=np.int64)[:, None]
    index = np.asarray(index, dtype=np.int64)
    n = index.shape[1]
    bits = grid.view(np.uint64)
    refine = _factor(ref_ratio, cell_level, level)
    at = lambda rel: (rel[2], rel[1], rel[0])
    value = np.full(n, _bits(fill), dtype=np.uint64)
    partial = np.zeros(n, dtype=bool)
    if cell_level < level:
        s = np.zeros(n, dtype=np.float64)
        count = np.zeros(n, dtype=np.int64)
        with np.errstate(all="ignore"):
            for kk in range(refine):
                for jj in range(refine):
                    for ii in range(refine):
                        rel = index * refine + np.array([[ii], [jj], [kk]], dtype=np.int64) - first
                        hit = np.all((rel >= 0) & (rel < dims), axis=0)
                        found = grid[at(np.where(hit, rel, 0))]
                        s = np.where(hit, s + found, s)
                        count += hit
            mean = s / np.where(count > 0, count, 1).astype(np.float64)
        inside = count > 0
        value[inside] = mean.view(np.uint64)[inside]
        partial = inside & (count < refine ** 3)
        return value.view(np.float64), ~inside, partial
    cell = index // refine                                  # floors, also below zero
    rel = cell - first
    inside = np.all((rel >= 0) & (rel < dims), axis=0)
    rel = np.where(inside, rel, 0)
    if cell_level == level or interpolation == 0:
        value[inside] = bits[at(rel)][inside]
        return value.view(np.float64), ~inside, partial
    centre = 2 * (index - cell * refine) + 1 - refine
    t = np.abs(centre).astype(np.float64) / np.float64(2 * refine)
    other = rel + np.where(centre < 0, -1, 1)
    low, high = other < 0, other >= dims
    if periodic:
        other = np.where(low, dims - 1, np.where(high, 0, other))
    else:
        other = np.where(low | high, rel, other)
    other = np.where(inside, other, 0)
    corner = lambda kz, jy, ix: grid[(other if kz else rel)[2], (other if jy else rel)[1],
                                     (other if ix else rel)[0]]
    with np.errstate(all="ignore"):
        step = lambda a, b, w: a + w * (b - a)              # rounded three times, nothing fused
        along_x = {(kz, jy): step(corner(kz, jy, 0), corner(kz, jy, 1), t[0])
                   for kz in (0, 1) for jy in (0, 1)}
        along_y = {kz: step(along_x[(kz, 0)], along_x[(kz, 1)], t[1]) for kz in (0, 1)}
        result = step(along_y[0], along_y[1], t[2])
    value[inside] = result.view(np.uint64)[inside]
    return value.view(np.float64), ~inside, partial


def grid_scene_of(arrays, ref_ratio, grid, level, lo, interpolation=0, periodic=False,
                  fill=np.nan):
    """arrays: leaf arrays of every level of the plotfile (an empty mask for a level that is not
    loaded).  Returns (dense, outside, partial): per level the values over the level's domain
    float64 [nz, ny, nx] (+0.0 where the cell is no leaf) and the two totals."""
    dense, outside, partial = [], 0, 0
    for l, (origin, mask, _) in enumerate(arrays):
        out = np.zeros(mask.shape, dtype=np.float64)
        k, j, i = np.nonzero(mask)
        if k.size:
            index = np.stack([i, j, k]).astype(np.int64) + origin[:, None]
            values, filled, part = grid_cells(grid, level, lo, l, index, ref_ratio, interpolation,
                                              periodic, fill)
            out.view(np.uint64)[k, j, i] = values.view(np.uint64)
            outside += int(filled.sum())
            partial += int(part.sum())
        dense.append(out)
    return dense, outside, partial


def grid_scene(levels, ref_ratio, grid, level, lo, interpolation=0, periodic=False, fill=np.nan,
               min_level=0, max_level=-1):
    """The same from a plotfile's own level arrays, as write_plotfile takes them."""
    arrays, _ = leaf_arrays(levels, ref_ratio, 0, min_level, max_level)
    return grid_scene_of(arrays, ref_ratio, grid, level, lo, interpolation, periodic, fill)
