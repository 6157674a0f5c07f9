"""Structure functions ("Structure functions"): what api.structure_functions works
out on the host around the kernel of csrc/avr_structure.hip -- the default lag vectors of a grid,
their rules, their physical lengths and unit directions, the bins over the lag length r, the
per-bin sums and moments, an .npz file.  numpy only; no device work."""
from __future__ import annotations

import itertools
import math
from typing import Dict, Optional, Tuple

import numpy as np

from . import spectra

MAX_LAGS = 4096            # csrc/avr_internal.h: kStructureMaxLags
MAX_ORDER = 8              # kStructureMaxOrder
MAX_BINS = spectra.MAX_BINS
VECTOR_KINDS = ("longitudinal", "transverse", "magnitude")   # the kinds of three components ...
SCALAR_KINDS = ("scalar",)                                    # ... and of one, in the kernel's order
# the 13 directions of the half space: of l and -l, which give the same pairs, the one whose first
# component that is not zero (x, then y, then z) is positive
_HALF_SPACE = tuple(u for u in itertools.product((0, 1, -1), repeat=3)
                    if next((c for c in u if c != 0), 0) > 0)


def kinds(n_components: int) -> Tuple[str, ...]:
    """The names of the kinds of increments of one or three components, in the kernel's order."""
    if n_components not in (1, 3):
        raise ValueError("a structure function takes one field or three")
    return SCALAR_KINDS if n_components == 1 else VECTOR_KINDS


def check_dims(dims) -> Tuple[int, int, int]:
    """dims = (nx, ny, nz) as ints; ValueError unless every one is at least 1 and there are fewer
    than 2^31 cells.  No power of two is asked for."""
    out = tuple(int(v) for v in dims)
    if len(out) != 3:
        raise ValueError("dims must hold three values")
    if min(out) < 1:
        raise ValueError(f"a structure function needs dims of at least 1, not {out}")
    if out[0] * out[1] * out[2] >= 1 << 31:
        raise ValueError(f"a structure function needs fewer than 2^31 cells, not {out}: pass a "
                         "smaller region or a coarser level")
    return out


def check_order(max_order) -> int:
    order = int(max_order)
    if not 1 <= order <= MAX_ORDER:
        raise ValueError(f"max_order must lie in [1, {MAX_ORDER}]")
    return order


def ladder(longest: int) -> list:
    """1, 2, 3, 4, 6, 8, 12, ...: the values 2^k and 3 * 2^(k - 1) up to `longest`, ascending."""
    steps, power = [], 1
    while power <= longest:
        steps.append(power)
        if power >= 2 and power + power // 2 <= longest:
            steps.append(power + power // 2)
        power *= 2
    return steps


def default_lags(dims) -> np.ndarray:
    """The default lags of a grid of dims = (nx, ny, nz), int32 [M, 3] rows (lx, ly, lz): the 13
    directions of a half space with components in {-1, 0, 1} -- those with a component along an
    axis of length 1 dropped -- times the ladder 1, 2, 3, 4, 6, 8, 12, ... up to min N_d // 2
    over the axes with N_d >= 2; direction by direction, each with its steps ascending.  182 lags
    for 256^3; none for a grid of one cell."""
    dims = check_dims(dims)
    wide = [d for d in range(3) if dims[d] >= 2]
    steps = ladder(min((dims[d] // 2 for d in wide), default=0))
    rows = [(step * u[0], step * u[1], step * u[2]) for u in _HALF_SPACE
            if all(u[d] == 0 or dims[d] >= 2 for d in range(3)) for step in steps]
    return np.array(rows, dtype=np.int32).reshape(-1, 3)


def check_lags(lags, dims) -> np.ndarray:
    """lags as contiguous int32 [M, 3]; ValueError unless 1 <= M <= 4096, no lag is zero and
    every |l_d| < N_d (a lag of a grid length would pair a cell with itself under periodic
    boundaries and with nothing otherwise)."""
    dims = check_dims(dims)
    given = np.asarray(lags)
    if given.ndim != 2 or given.shape[1] != 3 or not 1 <= given.shape[0] <= MAX_LAGS:
        raise ValueError(f"lags must be [M, 3] integers with M in [1, {MAX_LAGS}]")
    if not np.issubdtype(given.dtype, np.integer):
        if not np.array_equal(given, np.trunc(given)):
            raise ValueError("lags must be integers")
    wide = given.astype(np.int64)
    if not (wide != 0).any(axis=1).all():
        raise ValueError("a lag is zero")
    if not (np.abs(wide) < np.array(dims, dtype=np.int64)).all():
        raise ValueError(f"every lag must be shorter than the grid along every axis: |l_d| < N_d "
                         f"for dims {dims}")
    return np.ascontiguousarray(wide, dtype=np.int32)


def lag_lengths(lags, cell_size) -> np.ndarray:
    """r of every lag in physical units, float64 [M]: r^2 = f64(lx)^2 dx^2 + f64(ly)^2 dy^2, then
    + f64(lz)^2 dz^2 -- the integer squares exact, every product and sum rounded once -- and r =
    sqrt(r^2)."""
    l = np.asarray(lags, dtype=np.int64).reshape(-1, 3).astype(np.float64)
    dx, dy, dz = spectra._sizes(cell_size)
    r2 = (l[:, 0] * l[:, 0]) * (dx * dx) + (l[:, 1] * l[:, 1]) * (dy * dy)
    r2 = r2 + (l[:, 2] * l[:, 2]) * (dz * dz)
    return np.sqrt(r2)


def unit_directions(lags, cell_size) -> np.ndarray:
    """u = (l_d dx_d) / r, float64 [M, 3]: the unit vector of every lag in physical space, along
    which the longitudinal increment is taken."""
    l = np.asarray(lags, dtype=np.int64).reshape(-1, 3).astype(np.float64)
    size = np.array(spectra._sizes(cell_size), dtype=np.float64)
    return np.ascontiguousarray((l * size) / lag_lengths(lags, cell_size)[:, None])


def check_edges(edges) -> np.ndarray:
    """edges over r as float64 [n + 1]: finite, from a value >= 0 on, strictly increasing, 1 <= n
    <= 2048 (spectra.check_edges' rules); ValueError otherwise."""
    return spectra.check_edges(edges)


def make_edges(r_lag, bins: Optional[int] = None, r_range=None, r_log: bool = False):
    """The edges api.structure_functions uses without explicit ones: None -- one bin per distinct
    r -- without bins and r_range (r_log must be off).  Otherwise `bins` bins (by default as many
    as there are distinct r, 2048 at the most) over r_range = (r_min, r_max), by default the
    smallest and the largest r of the lags, evenly spaced, or with r_log in equal ratios."""
    if bins is None and r_range is None:
        if r_log:
            raise ValueError("r_log needs bins or r_range")
        return None
    r = np.asarray(r_lag, dtype=np.float64)
    bins = min(int(np.unique(r).size), MAX_BINS) if bins is None else int(bins)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"bins must lie in [1, {MAX_BINS}]")
    if r_range is None:
        r_range = (float(r.min()), float(r.max()))
        if r_range[0] == r_range[1]:      # one length: a bin around it
            r_range = (0.5 * r_range[0], 1.5 * r_range[1])
    lo, hi = (float(v) for v in r_range)
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 <= lo < hi):
        raise ValueError("r_range must be (r_min, r_max) with 0 <= r_min < r_max, both finite")
    if r_log:
        if lo <= 0.0:
            raise ValueError("r_log needs an r_min above 0")
        return np.geomspace(lo, hi, bins + 1)
    return np.linspace(lo, hi, bins + 1)


def bin_lags(r_lag, pairs_lag, sums_lag, edges=None) -> Dict:
    """The per-lag results gathered over r.  r_lag float64 [M], pairs_lag int64 [M], sums_lag
    float64 [M, K, P].  Without edges one bin per distinct r, ascending, the lags of bit-equal r
    grouped; with edges [n + 1] the joint histogram's rule: a lag lies in bin i when e[i] <= r <
    e[i + 1], the last bin closed at the top, and a lag beyond the edges is left out and counted.
    Per bin the pairs and the sums of its lags are added in lag order, and S = sums / pairs (NaN
    for a bin without pairs).  Returns a dict: r [n] (the distinct lengths, or the bins' centres),
    pairs int64 [n], sums float64 [n, K, P], S float64 [K, P, n], lags_outside."""
    r = np.ascontiguousarray(r_lag, dtype=np.float64)
    pairs_lag = np.ascontiguousarray(pairs_lag, dtype=np.int64)
    sums_lag = np.ascontiguousarray(sums_lag, dtype=np.float64)
    if r.ndim != 1 or pairs_lag.shape != r.shape or sums_lag.ndim != 3 or \
            sums_lag.shape[0] != r.size:
        raise ValueError("r_lag [M], pairs_lag [M] and sums_lag [M, K, P] must agree")
    if edges is None:
        centres, which = np.unique(r, return_inverse=True)
        which = which.reshape(-1)
    else:
        e = check_edges(edges)
        centres = 0.5 * (e[:-1] + e[1:])
        which = np.searchsorted(e, r, side="right") - 1
        which[r == e[-1]] = e.size - 2
        which[(r < e[0]) | (r > e[-1])] = -1
    n = int(centres.size)
    pairs = np.zeros(n, dtype=np.int64)
    sums = np.zeros((n,) + sums_lag.shape[1:], dtype=np.float64)
    outside = 0
    for m, b in enumerate(which.tolist()):
        if b < 0:
            outside += 1
            continue
        pairs[b] += pairs_lag[m]
        sums[b] = sums[b] + sums_lag[m]
    with np.errstate(divide="ignore", invalid="ignore"):
        moments = np.where(pairs[:, None, None] > 0,
                           sums / pairs[:, None, None].astype(np.float64), math.nan)
    return {"r": centres, "pairs": pairs, "sums": sums,
            "S": np.ascontiguousarray(np.moveaxis(moments, 0, -1)), "lags_outside": outside}


_INTS = ("level", "outside", "nonfinite", "absent", "max_order", "lags_outside")
_TUPLES = ("lo", "dims", "cell_size")


def save_npz(result: Dict, filename: str) -> None:
    """Writes api.structure_functions' dict as one .npz (numpy.savez): every entry under its key,
    the moments under "S/" + the kind."""
    entries = {}
    for key, value in result.items():
        if key == "S":
            for kind, array in value.items():
                entries[f"S/{kind}"] = np.asarray(array)
        else:
            entries[key] = np.asarray(value)
    with open(filename, "wb") as out:      # a file object: savez adds no ".npz" of its own
        np.savez(out, **entries)


def load_npz(filename: str) -> Dict:
    """Reads a file save_npz wrote back into a dict of the same shape: arrays stay arrays, level,
    max_order and the counts become ints, periodic a bool, fields a tuple of names, lo, dims and
    cell_size tuples."""
    result: Dict = {}
    with np.load(filename) as data:
        for key in data.files:
            head, _, name = key.partition("/")
            if head == "S" and name:
                result.setdefault("S", {})[name] = data[key]
            else:
                result[key] = data[key]
    for key in _INTS:
        if key in result:
            result[key] = int(result[key])
    for key in _TUPLES:
        if key in result:
            result[key] = tuple(result[key].tolist())
    if "periodic" in result:
        result["periodic"] = bool(result["periodic"])
    if "fields" in result:
        result["fields"] = tuple(str(name) for name in result["fields"].tolist())
    return result
