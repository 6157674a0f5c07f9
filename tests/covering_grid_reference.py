"""The reference of the covering grids ("Covering grid"): plain numpy on a plotfile's
own level arrays, as gradient_reference.leaf_arrays gives them (per level the origin, the leaf mask
and the values over the level's domain).  It never sees the scene's boxes.

The output cell with the level-L index G:
  1. for m = L, L - 1, ..., 0: G mapped to level m by floor division; the first level at which it
     is a leaf gives the value (bits kept), coverage 1.0 and the cell level m;
  2. else num = den = +0.0 and, for m = L + 1, ... in ascending order, R = ratio[L] ... ratio[m - 1],
     w = 1.0 / f64(R^3), s = +0.0, n = 0; for kk, then jj, then ii ascending in [0, R) the child
     R G + (ii, jj, kk), if a leaf of level m, gives s = s + v and n += 1; with n > 0: num = num +
     w * s, den = den + w * f64(n), cell level m.  With den > 0: value num / den, coverage den;
  3. else the fill value, coverage 0.0, cell level -1.
Vectorised over the output cells; the loops over m, kk, jj, ii keep the order of the additions.
"""
import numpy as np

from gradient_reference import _lookup, leaf_arrays


def covering_grid_of(arrays, ref_ratio, level, lo, dims, fill=np.nan):
    """arrays: leaf arrays of every level of the plotfile (an empty mask for a level that is not
    loaded); lo, dims = (nx, ny, nz): level-`level` indices.  Returns a dict: values, coverage
    float64 [nz, ny, nx], level int8 [nz, ny, nx] and levels_used int64 [nz, ny, nx], the number
    of levels that gave the cell a leaf."""
    nx, ny, nz = (int(v) for v in dims)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    index = np.stack([i.reshape(-1), j.reshape(-1), k.reshape(-1)]).astype(np.int64)
    index += np.array([int(v) for v in lo], dtype=np.int64)[:, None]
    n = index.shape[1]
    fill_bits = np.array([fill], dtype=np.float64).view(np.uint64)[0]
    value = np.full(n, fill_bits, dtype=np.uint64).view(np.float64)
    coverage = np.zeros(n, dtype=np.float64)
    cell_level = np.full(n, -1, dtype=np.int8)
    used = np.zeros(n, dtype=np.int64)
    present = np.zeros(n, dtype=bool)
    mapped = index.copy()
    for m in range(level, -1, -1):
        if m < level:
            mapped = mapped // ref_ratio[m]             # floors, also below zero
        hit, found = _lookup(arrays, m, mapped)
        take = hit & ~present
        value[take] = found[take]
        coverage[take] = 1.0
        cell_level[take] = m
        used[take] = 1
        present |= hit
    num = np.zeros(n, dtype=np.float64)
    den = np.zeros(n, dtype=np.float64)
    refine = 1
    with np.errstate(all="ignore"):
        for m in range(level + 1, len(arrays)):
            refine *= int(ref_ratio[m - 1])
            w = np.float64(1.0 / float(refine ** 3))
            s = np.zeros(n, dtype=np.float64)
            count = np.zeros(n, dtype=np.int64)
            for kk in range(refine):
                for jj in range(refine):
                    for ii in range(refine):
                        child = index * refine + np.array([[ii], [jj], [kk]], dtype=np.int64)
                        hit, found = _lookup(arrays, m, child)
                        s = np.where(hit, s + found, s)
                        count += hit
            has = (count > 0) & ~present
            product = w * s                              # rounded, then added: nothing fused
            num = np.where(has, num + product, num)
            den = np.where(has, den + w * count.astype(np.float64), den)
            cell_level[has] = m
            used[has] += 1
        averaged = ~present & (den > 0.0)
        quotient = num / np.where(averaged, den, 1.0)
    value[averaged] = quotient[averaged]
    coverage[averaged] = den[averaged]
    shape = (nz, ny, nx)
    return {"values": value.reshape(shape), "coverage": coverage.reshape(shape),
            "level": cell_level.reshape(shape), "levels_used": used.reshape(shape)}


def covering_grid(levels, ref_ratio, component, level, lo, dims, fill=np.nan, min_level=0,
                  max_level=-1):
    """The same from a plotfile's own level arrays, as write_plotfile takes them."""
    arrays, _ = leaf_arrays(levels, ref_ratio, component, min_level, max_level)
    return covering_grid_of(arrays, ref_ratio, level, lo, dims, fill)


def whole_domain(levels, ref_ratio, level):
    """(lo, dims) of level 0's domain refined to `level`."""
    refine = int(np.prod([int(r) for r in ref_ratio[:level]], dtype=np.int64)) if level else 1
    dlo, dhi = levels[0]["domain"]
    lo = tuple(int(v) * refine for v in dlo)
    return lo, tuple((int(dhi[a]) + 1) * refine - lo[a] for a in range(3))


def class_counts(result):
    """{cell level: number of cells}, -1 for the absent ones."""
    found, counts = np.unique(result["level"], return_counts=True)
    return {int(l): int(c) for l, c in zip(found, counts)}
