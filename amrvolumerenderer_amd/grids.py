"""Grids ("Covering grid"): what api.covering_grid works out on the host around the
arrays of csrc/avr_covering_grid.hip -- the cells of a level that a physical range selects, the
physical edges of a range of cells, an .npz file.  numpy only; no device work."""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np

_FIELD = "fields/"          # a field's entry in the .npz: this + its name


def _triple(values, what: str) -> Tuple[float, float, float]:
    out = tuple(float(v) for v in values)
    if len(out) != 3 or not all(math.isfinite(v) for v in out):
        raise ValueError(f"{what} must hold three finite values")
    return out


def index_region(prob_lo, cell_size, left_edge, right_edge):
    """The cells of a level whose centres lie in [left_edge, right_edge): (lo, dims), the index of
    the first cell and the number of cells per axis.  The centre of cell i is prob_lo + (i + 0.5)
    * cell_size in float64, and that very number is compared, so a cell is in exactly when its
    centre as api.covering_grid reports it is.  The range may leave the domain and lie below
    prob_lo (negative indices).  ValueError for a range that is not finite, holds no centre along
    some axis, or leaves 32 bits."""
    origin, size = _triple(prob_lo, "prob_lo"), _triple(cell_size, "cell_size")
    left, right = _triple(left_edge, "left_edge"), _triple(right_edge, "right_edge")
    if any(s <= 0.0 for s in size):
        raise ValueError("cell_size must be positive")
    lo, dims = [], []
    for a in range(3):
        def first_at_or_above(edge):
            """the smallest i whose centre is >= edge"""
            q = (edge - origin[a]) / size[a] - 0.5
            if not abs(q) < 2.0 ** 31:
                raise ValueError("the range leaves the 32-bit indices of its level")
            i = math.ceil(q)
            centre = lambda i: origin[a] + (i + 0.5) * size[a]
            while centre(i - 1) >= edge:
                i -= 1
            while centre(i) < edge:
                i += 1
            return i
        begin, end = first_at_or_above(left[a]), first_at_or_above(right[a])
        if end <= begin:
            raise ValueError("the range holds no cell centre along axis %d" % a)
        lo.append(begin)
        dims.append(end - begin)
    return tuple(lo), tuple(dims)


def grid_edges(prob_lo, cell_size, lo, dims):
    """(left_edge, right_edge) of the cells [lo, lo + dims): the low face of the first cell and the
    high face of the last, prob_lo + index * cell_size in float64."""
    origin, size = _triple(prob_lo, "prob_lo"), _triple(cell_size, "cell_size")
    left = tuple(origin[a] + int(lo[a]) * size[a] for a in range(3))
    right = tuple(origin[a] + (int(lo[a]) + int(dims[a])) * size[a] for a in range(3))
    return left, right


def save_npz(grid: Dict, filename: str) -> None:
    """Writes api.covering_grid's dict as one .npz (numpy.savez): every entry under its key, a
    field under "fields/" + its name."""
    entries = {key: np.asarray(value) for key, value in grid.items() if key != "fields"}
    for name, values in grid.get("fields", {}).items():
        entries[_FIELD + str(name)] = np.asarray(values, dtype=np.float64)
    with open(filename, "wb") as out:      # a file object: savez adds no ".npz" of its own
        np.savez(out, **entries)


def load_npz(filename: str) -> Dict:
    """Reads a file save_npz wrote back into a dict of the same shape: arrays stay arrays, level,
    absent and partial become ints, lo, dims and the edges tuples."""
    grid: Dict = {"fields": {}}
    with np.load(filename) as data:
        for key in data.files:
            if key.startswith(_FIELD):
                grid["fields"][key[len(_FIELD):]] = data[key]
            else:
                grid[key] = data[key]
    for key in ("level", "absent", "partial"):
        if key in grid:
            grid[key] = int(grid[key])
    for key in ("lo", "dims", "left_edge", "right_edge", "cell_size"):
        if key in grid:
            grid[key] = tuple(grid[key].tolist())
    return grid
