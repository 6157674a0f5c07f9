"""Rays ("Rays"): what api.rays works out on the host around the arrays of
csrc/avr_rays.hip -- the end points as arrays, the default trip bound, the points in the middle of
the segments, an .npz file -- and around the per-ray sums of an off-axis projection (DESIGN.md 7,
"Off-axis projection"): the rays of an image's pixels and the order that lists them tile by tile.
numpy only; no device work."""
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


PIXEL_TILE = 8          # pixel_order's tiles are 8 x 8: the 64 lanes of a wave


def pixel_rays(center, n, U, V, plane_width, depth, width: int,
               height: int) -> Tuple[np.ndarray, np.ndarray]:
    """(start, end), float64 [height * width, 3] in row-major pixel order with row 0 at the
    bottom: the rays of an orthographic image ("Off-axis projection").  Pixel (x, y)
    owns the point P[d] = (center[d] + su U[d]) + sv V[d] of the image plane, su = ((x + 0.5) /
    width - 0.5) wu, sv = ((y + 0.5) / height - 0.5) wv, (wu, wv) = plane_width; its ray runs from
    P + h n to P - h n, h = 0.5 depth -- away from the viewer that n points at.  Plain float64 in
    the order written here."""
    width, height = int(width), int(height)
    if width <= 0 or height <= 0:
        raise ValueError("image dimensions must be positive")
    center, n, U, V = (np.asarray(v, dtype=np.float64).reshape(3) for v in (center, n, U, V))
    wu, wv = (np.float64(w) for w in plane_width)
    su = ((np.arange(width, dtype=np.float64) + 0.5) / np.float64(width) - 0.5) * wu
    sv = ((np.arange(height, dtype=np.float64) + 0.5) / np.float64(height) - 0.5) * wv
    h = 0.5 * np.float64(depth)
    start = np.empty((height, width, 3), dtype=np.float64)
    end = np.empty((height, width, 3), dtype=np.float64)
    for d in range(3):
        P = (center[d] + su[None, :] * U[d]) + sv[:, None] * V[d]
        start[:, :, d] = P + h * n[d]
        end[:, :, d] = P - h * n[d]
    return start.reshape(-1, 3), end.reshape(-1, 3)


def pixel_order(width: int, height: int) -> np.ndarray:
    """The int64 permutation of the row-major pixel numbers y * width + x that lists the pixels
    tile by tile: tiles of 8 x 8 pixels taken row-major, the pixels inside a tile row-major, those
    outside the image dropped.  64 rays in a row are then a compact block of the image where the
    width is a multiple of 8."""
    width, height = int(width), int(height)
    if width <= 0 or height <= 0:
        raise ValueError("image dimensions must be positive")
    t = PIXEL_TILE
    tiles_x, tiles_y = (width + t - 1) // t, (height + t - 1) // t
    ty, tx, py, px = np.meshgrid(np.arange(tiles_y), np.arange(tiles_x), np.arange(t),
                                 np.arange(t), indexing="ij")
    x, y = (tx * t + px).reshape(-1), (ty * t + py).reshape(-1)
    inside = (x < width) & (y < height)
    return (y[inside] * width + x[inside]).astype(np.int64)


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
