"""The host side of velocity cubes ("Velocity cubes"), in numpy: the argument checks
of api.velocity_cube, the channel edges, the sum over owners, the moment maps and the two file
formats (.npz and a minimal FITS writer in pure Python).  Nothing here touches the device."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import numpy as np

MAX_CHANNELS = 1024
_AXES = ("x", "y", "z")
FITS_BLOCK = 2880


def _name(value, what: str, optional: bool = False) -> None:
    if value is None and optional:
        return
    if not isinstance(value, str) or not value:
        raise ValueError(f"{what} must be a variable name{' or None' if optional else ''}, "
                         f"not {value!r}")


def checked_edges(edges):
    """edges as a float64 array: 2 .. 1025 finite, strictly increasing values."""
    e = np.array(edges, dtype=np.float64)
    if e.ndim != 1 or not (2 <= e.size <= MAX_CHANNELS + 1):
        raise ValueError(f"edges must hold between 2 and {MAX_CHANNELS + 1} values")
    if not np.isfinite(e).all():
        raise ValueError("edges must be finite")
    if not (e[1:] > e[:-1]).all():
        raise ValueError("edges must be strictly increasing")
    return e


def validate_cube_arguments(axis: str = "z", emission: Optional[str] = None,
                            velocity: Optional[str] = None, width_field: Optional[str] = None,
                            channels: int = 64, v_range: Optional[Sequence[float]] = None,
                            edges=None, width: int = 256, height: int = 256,
                            center: Optional[Sequence[float]] = None,
                            plane_width: Optional[Sequence[float]] = None,
                            output: Optional[str] = None):
    """The argument checks of api.velocity_cube, before any GPU work and before the plotfile is
    opened.  Returns (center or None, plane_width or None, v_range or None, edges or None) as
    floats; explicit edges override channels and v_range."""
    import operator
    if axis not in _AXES:
        raise ValueError(f"axis must be one of x, y, z, not {axis!r}")
    _name(emission, "emission")
    _name(velocity, "velocity")
    _name(width_field, "width_field", optional=True)
    for name, size in (("width", width), ("height", height)):
        try:
            size = operator.index(size)
        except TypeError:
            size = 0
        if isinstance(size, bool) or size <= 0:
            raise ValueError(f"{name} must be a positive integer")
    if center is not None:
        center = tuple(float(c) for c in center)
        if len(center) != 3 or not all(math.isfinite(c) for c in center):
            raise ValueError("center must hold three finite values")
    widths = None
    if plane_width is not None:
        widths = tuple(float(v) for v in plane_width)
        if len(widths) != 2:
            raise ValueError("plane_width must hold two values (wu, wv)")
        if not all(math.isfinite(v) and v > 0.0 for v in widths):
            raise ValueError("plane_width must be finite and positive")
    rng = None
    if edges is not None:
        edges = checked_edges(edges)
        n = edges.size - 1
    else:
        try:
            n = operator.index(channels)
        except TypeError:
            n = 0
        if isinstance(channels, bool) or not (1 <= n <= MAX_CHANNELS):
            raise ValueError(f"channels must be an integer in [1, {MAX_CHANNELS}]")
        if v_range is not None:
            rng = tuple(float(v) for v in v_range)
            if len(rng) != 2:
                raise ValueError("v_range must hold two values (lo, hi)")
            if not (math.isfinite(rng[0]) and math.isfinite(rng[1]) and rng[0] < rng[1]):
                raise ValueError("v_range must be finite with lo < hi")
            channel_edges(rng, n)       # a range too narrow for the channels is refused here
    if int(n) * int(width) * int(height) >= 2 ** 31:
        raise ValueError("the cube has 2^31 entries or more")
    if output is not None:
        if not isinstance(output, str) or not output.lower().endswith((".npz", ".fits")):
            raise ValueError("output must end in .npz or .fits")
        if output.lower().endswith(".fits") and edges is not None:
            channel_spacing(edges)      # FITS has a linear channel axis only
    return center, widths, rng, edges


def channel_edges(v_range: Sequence[float], channels: int):
    """The channels + 1 linear edges over v_range = (lo, hi): api.bin_edges."""
    from . import api
    lo, hi = v_range
    return api.bin_edges(lo, hi, channels)


def channel_centers(edges):
    e = np.asarray(edges, dtype=np.float64)
    return 0.5 * (e[:-1] + e[1:])


def combine_velocity_cubes(parts):
    """The cubes of several owners -> that of them all: the plain sum, in the order given.
    parts: (cube, under, over, length) tuples as Scene.velocity_cube returns them (torch tensors
    or numpy arrays, the same shapes in every part)."""
    parts = list(parts)
    if not parts:
        raise ValueError("combine_velocity_cubes needs at least one part")
    total = [a.copy() if hasattr(a, "copy") else a.clone() for a in parts[0]]
    if len(total) != 4:
        raise ValueError("a part is (cube, under, over, length)")
    for part in parts[1:]:
        if len(part) != 4 or any(tuple(a.shape) != tuple(t.shape) for a, t in zip(part, total)):
            raise ValueError("parts must agree in shape")
        for t, a in zip(total, part):
            t += a
    return tuple(total)


def moments(cube, edges):
    """(moment 0, moment 1, moment 2) of cube [nc, H, W] over the channel centres v_c = (e[c] +
    e[c + 1]) / 2: moment 0 = sum_c cube, moment 1 = sum_c cube v_c / moment 0 (the centroid),
    moment 2 = sqrt(max(sum_c cube (v_c - moment 1)^2 / moment 0, 0)) (the dispersion); moments 1
    and 2 are NaN where moment 0 is 0.  float64 [H, W] each."""
    cube = np.asarray(cube, dtype=np.float64)
    e = checked_edges(edges)
    if cube.ndim != 3 or cube.shape[0] != e.size - 1:
        raise ValueError("cube must be [channels, height, width] with channels + 1 edges")
    v = channel_centers(e)[:, None, None]
    m0 = cube.sum(axis=0)
    filled = m0 != 0.0
    safe = np.where(filled, m0, 1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        m1 = (cube * v).sum(axis=0) / safe
        m2 = np.sqrt(np.maximum((cube * (v - m1) ** 2).sum(axis=0) / safe, 0.0))
    nan = np.full_like(m0, np.nan)
    return m0, np.where(filled, m1, nan), np.where(filled, m2, nan)


def write_npz(path: str, result: dict,
              keys: Sequence[str] = ("cube", "under", "over", "length", "edges", "centers")) -> None:
    """The arrays of api.velocity_cube's dict -> an .npz (moments as moment0, moment1, moment2).
    keys: the arrays of another cube's dict (api.line_cube)."""
    arrays = {k: np.asarray(result[k]) for k in keys}
    for i, m in enumerate(result["moments"]):
        arrays[f"moment{i}"] = np.asarray(m)
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def channel_spacing(edges) -> float:
    """The common width of uniformly spaced channels; ValueError if the edges are not uniform
    (to 8 ulp of the largest edge, what api.bin_edges' linear edges keep)."""
    e = checked_edges(edges)
    step = (e[-1] - e[0]) / (e.size - 1)
    slack = 8.0 * np.finfo(np.float64).eps * max(abs(e[0]), abs(e[-1]))
    if not (np.abs(np.diff(e) - step) <= slack).all():
        raise ValueError("a FITS cube needs uniformly spaced channel edges")
    return float(step)


def _card(key: str, value, comment: str = "") -> bytes:
    if isinstance(value, bool):
        text = ("T" if value else "F").rjust(20)
    elif isinstance(value, int):
        text = str(value).rjust(20)
    elif isinstance(value, float):
        text = f"{value:.17G}"
        if "." not in text and "E" not in text:
            text += "."
        text = text.rjust(20)
    else:
        text = ("'" + str(value).replace("'", "''").ljust(8) + "'").ljust(20)
    card = f"{key:<8}= {text}" + (f" / {comment}" if comment else "")
    if len(card) > 80:
        card = card[:80]
    return card.ljust(80).encode("ascii")


def write_fits(path: str, cube, edges, origin_uv: Sequence[float] = (0.0, 0.0),
               pixel_size: Sequence[float] = (1.0, 1.0), axis: str = "z",
               bunit: Optional[str] = None) -> None:
    """cube [nc, H, W] -> a FITS file with one primary HDU: 2880-byte blocks, BITPIX = -64,
    big-endian, NAXIS = 3 with NAXIS1 = W, NAXIS2 = H, NAXIS3 = nc (row 0 at the bottom, as FITS
    has it).  Linear WCS: pixel x has its centre at origin_uv[0] + (x + 0.5) pixel_size[0], so
    CRPIX1 = 1, CRVAL1 = origin_uv[0] + pixel_size[0] / 2, CDELT1 = pixel_size[0], likewise axis 2;
    axis 3 is the channel centre, CRPIX3 = 1, CRVAL3 = (edges[0] + edges[1]) / 2, CDELT3 = the
    channel width.  CTYPE1 / CTYPE2 name the image axes of `axis` ((y, z), (z, x), (x, y)),
    CTYPE3 = 'VELO'.  ValueError for edges that are not uniformly spaced."""
    data = np.asarray(cube, dtype=np.float64)
    e = checked_edges(edges)
    if data.ndim != 3 or data.shape[0] != e.size - 1:
        raise ValueError("cube must be [channels, height, width] with channels + 1 edges")
    if axis not in _AXES:
        raise ValueError(f"axis must be one of x, y, z, not {axis!r}")
    step = channel_spacing(e)
    a = _AXES.index(axis)
    names = (_AXES[(a + 1) % 3].upper(), _AXES[(a + 2) % 3].upper())
    ou, ov = (float(v) for v in origin_uv)
    du, dv = (float(v) for v in pixel_size)
    nc, height, width = data.shape
    cards = [_card("SIMPLE", True, "conforms to FITS"), _card("BITPIX", -64, "IEEE binary64"),
             _card("NAXIS", 3), _card("NAXIS1", int(width)), _card("NAXIS2", int(height)),
             _card("NAXIS3", int(nc)),
             _card("CTYPE1", names[0]), _card("CRPIX1", 1.0), _card("CRVAL1", ou + 0.5 * du),
             _card("CDELT1", du),
             _card("CTYPE2", names[1]), _card("CRPIX2", 1.0), _card("CRVAL2", ov + 0.5 * dv),
             _card("CDELT2", dv),
             _card("CTYPE3", "VELO"), _card("CRPIX3", 1.0),
             _card("CRVAL3", float(0.5 * (e[0] + e[1]))), _card("CDELT3", step)]
    if bunit is not None:
        cards.append(_card("BUNIT", str(bunit)))
    cards.append(b"END".ljust(80))
    header = b"".join(cards)
    header += b" " * (-len(header) % FITS_BLOCK)
    body = np.ascontiguousarray(data, dtype=">f8").tobytes()
    body += b"\0" * (-len(body) % FITS_BLOCK)
    with open(path, "wb") as f:
        f.write(header)
        f.write(body)
