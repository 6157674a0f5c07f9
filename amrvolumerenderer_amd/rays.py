"""Rays ("Rays"): what api.rays works out on the host around the arrays of
csrc/avr_rays.hip -- the end points as arrays, the default trip bound, the points in the middle of
the segments, an .npz file.  numpy only; no device work."""
from __future__ import annotations

from typing import Dict, Sequence, Tuple

import numpy as np

MAX_TRIPS = 2 ** 30
COMPLETE, MISS, TRUNCATED, INVALID = 0, 1, 2, 3      # a ray's status byte
_FIELD, _INTEGRAL = "fields/", "integrals/"          # a field's entries in the .npz: this + its name


def end_points(start, end) -> Tuple[np.ndarray, np.ndarray]:
    """start and end as float64 [n, 3]: each is [n, 3], or a single [3]."""
    out = []
    for points, what in ((start, "start"), (end, "end")):
        points = np.ascontiguousarray(points, dtype=np.float64)
        if points.ndim == 1 and points.shape[0] == 3:
            points = points.reshape(1, 3)
        if points.ndim != 2 or points.shape[1] != 3:
            raise ValueError(f"{what} must be an array [n, 3], or one point [3]")
        out.append(points)
    if out[0].shape != out[1].shape:
        raise ValueError("start and end must hold the same number of points")
    return out[0], out[1]


def level0_bounds(index_lo, dims, levels, ref_ratio):
    """(Blo, Bhi): the level-0 index bounding box of the boxes that have cells, every box mapped
    to level 0 by floor division (box b: first cell index_lo[b], dims[b] = (nx, ny, nz) cells,
    level levels[b]); None for a scene without cells."""
    lo = hi = None
    for first, extent, level in zip(index_lo, dims, levels):
        if min(int(v) for v in extent) <= 0:
            continue
        box_lo = [int(v) for v in first]
        box_hi = [int(v) + int(n) - 1 for v, n in zip(first, extent)]
        for m in range(int(level), 0, -1):
            r = int(ref_ratio[m - 1])
            box_lo = [v // r for v in box_lo]
            box_hi = [v // r for v in box_hi]
        lo = box_lo if lo is None else [min(a, b) for a, b in zip(lo, box_lo)]
        hi = box_hi if hi is None else [max(a, b) for a, b in zip(hi, box_hi)]
    return None if lo is None else (tuple(lo), tuple(hi))


def default_max_trips(bounds, ref_ratio: Sequence[int], n_levels: int) -> int:
    """8 + 2 sum_d (Bhi[d] - Blo[d] + 1) (r_0 ... r_(n_levels - 2)): twice the planes of the finest
    level that a ray can cross, 2^30 at the most."""
    if bounds is None:
        return 8
    refine = 1
    for r in list(ref_ratio)[:max(int(n_levels) - 1, 0)]:
        refine *= int(r)
    planes = sum(hi - lo + 1 for lo, hi in zip(*bounds)) * refine
    return min(8 + 2 * planes, MAX_TRIPS)


def segment_midpoints(result: Dict) -> np.ndarray:
    """The point A + 0.5 (t0 + t1) (B - A) of every segment of api.rays' dict, float64 [total, 3]:
    where to sample another product along the rays."""
    start, end = end_points(result["start"], result["end"])
    offsets = np.asarray(result["offsets"], dtype=np.int64)
    ray = np.repeat(np.arange(offsets.size - 1), np.diff(offsets))
    t = 0.5 * (np.asarray(result["t0"], dtype=np.float64) + np.asarray(result["t1"],
                                                                        dtype=np.float64))
    return start[ray] + t[:, None] * (end[ray] - start[ray])


def save_npz(result: Dict, filename: str) -> None:
    """Writes api.rays' dict as one .npz (numpy.savez): every entry under its key, a field's
    values under "fields/" + its name and its integrals under "integrals/" + its name."""
    entries = {key: np.asarray(value) for key, value in result.items()
               if key not in ("fields", "integrals")}
    for name, values in result.get("fields", {}).items():
        entries[_FIELD + str(name)] = np.asarray(values, dtype=np.float64)
    for name, values in result.get("integrals", {}).items():
        entries[_INTEGRAL + str(name)] = np.asarray(values, dtype=np.float64)
    with open(filename, "wb") as out:      # a file object: savez adds no ".npz" of its own
        np.savez(out, **entries)


def load_npz(filename: str) -> Dict:
    """Reads a file save_npz wrote back into a dict of the same shape: arrays stay arrays, n
    becomes an int."""
    result: Dict = {"fields": {}, "integrals": {}}
    with np.load(filename) as data:
        for key in data.files:
            if key.startswith(_FIELD):
                result["fields"][key[len(_FIELD):]] = data[key]
            elif key.startswith(_INTEGRAL):
                result["integrals"][key[len(_INTEGRAL):]] = data[key]
            else:
                result[key] = data[key]
    if "n" in result:
        result["n"] = int(result["n"])
    return result
