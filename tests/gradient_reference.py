"""The reference of the gradient fields ("Gradient fields"): plain numpy on a
plotfile's own level arrays, as write_plotfile takes them (levels[l] = {"domain", "boxes", "data":
[array [ncomp, nz, ny, nx]]}).

Per loaded level a leaf mask and the leaf values over the level's domain, in that level's index
space: a cell is a leaf of level l if a grid of level l holds it, min_level <= l <= max_level, and
(l == max_level or no grid of level l + 1, coarsened by floor division, covers it).  A cell's
neighbour one step along the axis is looked up as the ghost rules say, whether or not it lies in
the cell's own box (inside the box it is a leaf of the same level, which rule 1 finds first):
  1. for m = l, l - 1, ..., 0: the neighbour's index mapped to level m by floor division; the first
     level at which it is a leaf gives the value;
  2. else, if level l + 1 is loaded and every one of the r^3 children r * G + (0 .. r - 1)^3 is a
     leaf of level l + 1: (0.0 + the children, one addition each, ascending k, then j, then i) /
     f64(r^3);
  3. else it is absent.
The value is (H - L) / (2.0 * dx), (H - f) / dx, (f - L) / dx or 0.0 by which neighbours exist.
"""
import numpy as np


def cell_sizes(levels, prob_lo, prob_hi):
    """[(dx, dy, dz)] per level from the level domains, as write_plotfile derives them."""
    out = []
    for lev in levels:
        lo, hi = lev["domain"]
        out.append(tuple((prob_hi[a] - prob_lo[a]) / (hi[a] - lo[a] + 1) for a in range(3)))
    return out


def same_bits(a, b):
    """Equal by bits, NaN equal to NaN."""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    both_nan = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | both_nan).all())


def leaf_arrays(levels, ref_ratio, component, min_level=0, max_level=-1):
    """Per level (origin (i, j, k), leaf mask [nz, ny, nx], values [nz, ny, nx]) over the level's
    domain; the mask of a level outside [min_level, max_level] is empty."""
    if max_level < 0 or max_level >= len(levels):
        max_level = len(levels) - 1
    out = []
    for l, lev in enumerate(levels):
        dlo, dhi = lev["domain"]
        shape = tuple(dhi[a] - dlo[a] + 1 for a in (2, 1, 0))
        mask = np.zeros(shape, dtype=bool)
        values = np.zeros(shape, dtype=np.float64)
        if min_level <= l <= max_level:
            for (lo, hi), data in zip(lev["boxes"], lev["data"]):
                cut = tuple(slice(lo[a] - dlo[a], hi[a] - dlo[a] + 1) for a in (2, 1, 0))
                mask[cut] = True
                values[cut] = np.asarray(data, dtype=np.float64)[component]
            if l < max_level:
                r = ref_ratio[l]
                for lo, hi in levels[l + 1]["boxes"]:
                    cut = tuple(slice(lo[a] // r - dlo[a], hi[a] // r - dlo[a] + 1)
                                for a in (2, 1, 0))
                    mask[cut] = False
        out.append((np.array(dlo, dtype=np.int64), mask, values))
    return out, max_level


def _lookup(arrays, level, index):
    """index [3, n] (i, j, k) of `level` -> (is a leaf [n], its value [n], junk where it is not)."""
    origin, mask, values = arrays[level]
    rel = index - origin[:, None]
    extent = np.array(mask.shape[::-1], dtype=np.int64)
    inside = np.all((rel >= 0) & (rel < extent[:, None]), axis=0)
    safe = np.where(inside, rel, 0)
    at = (safe[2], safe[1], safe[0])
    return inside & mask[at], values[at]


def neighbour(arrays, ref_ratio, level, index, max_level):
    """The three ghost rules for the level-`level` indices index [3, n] -> (present, value)."""
    n = index.shape[1]
    present = np.zeros(n, dtype=bool)
    value = np.zeros(n, dtype=np.float64)
    mapped = index.copy()
    for m in range(level, -1, -1):
        if m < level:
            mapped = mapped // ref_ratio[m]             # floors, also below zero
        hit, found = _lookup(arrays, m, mapped)
        take = hit & ~present
        value[take] = found[take]
        present |= hit
    if level + 1 <= max_level:
        r = ref_ratio[level]
        every = np.ones(n, dtype=bool)
        total = np.zeros(n, dtype=np.float64)
        with np.errstate(all="ignore"):
            for kk in range(r):
                for jj in range(r):
                    for ii in range(r):
                        child = index * r + np.array([[ii], [jj], [kk]], dtype=np.int64)
                        hit, found = _lookup(arrays, level + 1, child)
                        every &= hit
                        total = total + found
            mean = total / np.float64(r ** 3)
        take = every & ~present
        value[take] = mean[take]
        present |= take
    return present, value


def gradient_levels(levels, ref_ratio, sizes, axis, component, min_level=0, max_level=-1):
    """Per level the difference along axis over the level's domain [nz, ny, nx] (0.0 where the
    cell is no leaf), and the leaf arrays it was computed from.  sizes[l] = (dx, dy, dz)."""
    arrays, max_level = leaf_arrays(levels, ref_ratio, component, min_level, max_level)
    out = []
    for l, (origin, mask, values) in enumerate(arrays):
        result = np.zeros(mask.shape, dtype=np.float64)
        k, j, i = np.nonzero(mask)
        if k.size:
            index = np.stack([i, j, k]).astype(np.int64) + origin[:, None]
            step = np.zeros((3, 1), dtype=np.int64)
            step[axis] = 1
            has_l, low = neighbour(arrays, ref_ratio, l, index - step, max_level)
            has_h, high = neighbour(arrays, ref_ratio, l, index + step, max_level)
            f = values[k, j, i]
            dx = np.float64(sizes[l][axis])
            with np.errstate(all="ignore"):
                both = (high - low) / (2.0 * dx)
                only_h = (high - f) / dx
                only_l = (f - low) / dx
            result[k, j, i] = np.where(has_l & has_h, both,
                                       np.where(has_h, only_h, np.where(has_l, only_l, 0.0)))
        out.append(result)
    return out, arrays


def brute_force(levels, ref_ratio, sizes, axis, component, min_level=0, max_level=-1):
    """The same definition cell by cell with dictionaries and Python floats: {(l, i, j, k): value}
    for every leaf."""
    if max_level < 0 or max_level >= len(levels):
        max_level = len(levels) - 1
    leaves = [dict() for _ in levels]
    for l in range(min_level, max_level + 1):
        for (lo, hi), data in zip(levels[l]["boxes"], levels[l]["data"]):
            for k in range(lo[2], hi[2] + 1):
                for j in range(lo[1], hi[1] + 1):
                    for i in range(lo[0], hi[0] + 1):
                        leaves[l][(i, j, k)] = float(data[component][k - lo[2], j - lo[1], i - lo[0]])
        if l < max_level:
            r = ref_ratio[l]
            for lo, hi in levels[l + 1]["boxes"]:
                for k in range(lo[2] // r, hi[2] // r + 1):
                    for j in range(lo[1] // r, hi[1] // r + 1):
                        for i in range(lo[0] // r, hi[0] // r + 1):
                            leaves[l].pop((i, j, k), None)

    def ghost(l, g):
        mapped = g
        for m in range(l, -1, -1):
            if m < l:
                mapped = tuple(v // ref_ratio[m] for v in mapped)
            if mapped in leaves[m]:
                return leaves[m][mapped]
        if l + 1 <= max_level:
            r = ref_ratio[l]
            total = np.float64(0.0)
            for kk in range(r):
                for jj in range(r):
                    for ii in range(r):
                        child = (g[0] * r + ii, g[1] * r + jj, g[2] * r + kk)
                        if child not in leaves[l + 1]:
                            return None
                        total = total + np.float64(leaves[l + 1][child])
            return total / np.float64(r ** 3)
        return None

    out = {}
    with np.errstate(all="ignore"):
        for l in range(len(levels)):
            dx = np.float64(sizes[l][axis])
            for cell, f in leaves[l].items():
                below = tuple(v - (a == axis) for a, v in enumerate(cell))
                above = tuple(v + (a == axis) for a, v in enumerate(cell))
                low, high, f = ghost(l, below), ghost(l, above), np.float64(f)
                if low is not None and high is not None:
                    value = (np.float64(high) - np.float64(low)) / (2.0 * dx)
                elif high is not None:
                    value = (np.float64(high) - f) / dx
                elif low is not None:
                    value = (f - np.float64(low)) / dx
                else:
                    value = np.float64(0.0)
                out[(l,) + cell] = float(value)
    return out


# ---- fixtures ------------------------------------------------------------------------------------

VARIABLES = ("u", "odd", "whole")
POISON = 1e30


def make_levels(domains, boxes, ref_ratio, seed):
    """levels for write_plotfile with three fields: u (normal), odd (u with about 2 % NaN / +Inf /
    -Inf) and whole (integers); every cell that a grid of the next level covers holds 1e30 in all
    three, so that a read of a parent grid past a leaf box's view shows."""
    rng = np.random.default_rng(seed)
    levels = []
    for l, (domain, grids) in enumerate(zip(domains, boxes)):
        data = []
        for lo, hi in grids:
            shape = (hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
            u = rng.standard_normal(shape)
            odd = u.copy().reshape(-1)
            pick = rng.choice(odd.size, min(max(odd.size // 50, 3), odd.size), replace=False)
            odd[pick] = np.array([np.nan, np.inf, -np.inf])[np.arange(pick.size) % 3]
            whole = rng.integers(-1000, 1001, size=shape).astype(np.float64)
            cells = np.stack([u, odd.reshape(shape), whole])
            if l + 1 < len(boxes):
                r = ref_ratio[l]
                for flo, fhi in boxes[l + 1]:
                    cut = tuple(slice(max(flo[a] // r, lo[a]) - lo[a],
                                      max(min(fhi[a] // r, hi[a]) - lo[a] + 1, 0)) for a in (2, 1, 0))
                    cells[(slice(None),) + cut] = POISON
            data.append(cells)
        levels.append({"domain": domain, "boxes": list(grids), "data": data})
    return levels
