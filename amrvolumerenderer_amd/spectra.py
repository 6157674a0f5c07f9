"""Power spectra ("Power spectrum"): what api.power_spectrum works out on the host
around the kernels of csrc/avr_fft.hip and csrc/avr_spectral.hip -- the wave numbers of a grid,
the default, linear and logarithmic edges, their squares as the bin kernel compares them, the
normalisation of the shell sums, an .npz file -- and, for api.helmholtz and api.potential
("Inverse transform, Helmholtz split, potential"), the inverse lengths, the
compressive fraction and their .npz files; for api.isolated_potential ("Isolated
potential") the padding rule and its .npz file.  numpy only; no device work."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

MAX_LENGTH = 1024          # per axis, a power of two (csrc/avr_internal.h: kFftMaxLength)
MAX_BINS = 2048            # kSpectrumMaxBins
_FIELD = "fields/"         # a field's entries in the .npz: this + its name + "/" + the entry
_ENTRIES = ("power", "spectrum", "modes")


def check_dims(dims) -> Tuple[int, int, int]:
    """dims = (nx, ny, nz) as ints; ValueError unless every one is a power of two in [1, 1024]."""
    out = tuple(int(v) for v in dims)
    if len(out) != 3:
        raise ValueError("dims must hold three values")
    for n in out:
        if not 1 <= n <= MAX_LENGTH or n & (n - 1):
            raise ValueError(f"a power spectrum needs dims that are powers of two in [1, "
                             f"{MAX_LENGTH}], not {out}: pass a region of such a size")
    return out


def _sizes(cell_size) -> Tuple[float, float, float]:
    out = tuple(float(v) for v in cell_size)
    if len(out) != 3 or not all(math.isfinite(v) and v > 0.0 for v in out):
        raise ValueError("cell_size must hold three finite, positive values")
    return out


def signed_modes(n: int) -> np.ndarray:
    """The signed wave number m of every index k of an axis of n modes (int64 [n]): k below n / 2
    or with n == 1, else k - n -- numpy.fft.fftfreq's convention."""
    k = np.arange(int(n), dtype=np.int64)
    return np.where((k < n // 2) | (n == 1), k, k - n)


def lengths(dims, cell_size) -> Tuple[float, float, float]:
    """L_d = N_d * cell_size_d in float64."""
    return tuple(float(n) * s for n, s in zip(check_dims(dims), _sizes(cell_size)))


def inverse_length_sq(dims, cell_size) -> np.ndarray:
    """g[d] = 1.0 / (L_d * L_d), float64 [3]: what the bin kernel multiplies m_d^2 by."""
    return np.array([1.0 / (length * length) for length in lengths(dims, cell_size)],
                    dtype=np.float64)


def inverse_length(dims, cell_size) -> np.ndarray:
    """h[d] = 1.0 / L_d, float64 [3]: what the Helmholtz kernel multiplies m_d by."""
    return np.array([1.0 / length for length in lengths(dims, cell_size)], dtype=np.float64)


def wave_numbers(dims, cell_size):
    """(kx [nx], ky [ny], kz [nz]): the physical wave number 2 pi m / L_d of every index."""
    return tuple(2.0 * math.pi * signed_modes(n).astype(np.float64) / length
                 for n, length in zip(check_dims(dims), lengths(dims, cell_size)))


def default_edges(dims, cell_size) -> np.ndarray:
    """The default edges: over the axes with N_d >= 2, dk = 2 pi / max L_d and n = min N_d // 2
    (0 without such an axis, where dk takes every axis); e[0] = 0 and e[i] = (i - 0.5) dk for
    1 <= i <= n + 1.  n + 1 bins: bin 0 holds the mean alone, bin i the modes within half a
    fundamental of i dk, up to the smallest Nyquist wave number."""
    dims = check_dims(dims)
    size = lengths(dims, cell_size)
    wide = [d for d in range(3) if dims[d] >= 2]
    dk = 2.0 * math.pi / max(size[d] for d in (wide or range(3)))
    n = min((dims[d] // 2 for d in wide), default=0)
    return np.array([0.0] + [(i - 0.5) * dk for i in range(1, n + 2)], dtype=np.float64)


def make_edges(dims, cell_size, bins: Optional[int] = None, k_range=None,
               k_log: bool = False) -> np.ndarray:
    """The edges api.power_spectrum uses without explicit ones.  Without bins and k_range, the
    default edges (k_log must be off).  Otherwise `bins` bins (by default as many as the default
    edges have) over k_range = (k_min, k_max), evenly spaced, or with k_log in equal ratios; by
    default k_range runs from the default edges' first (0) -- with k_log their second, half a
    fundamental -- to their last."""
    default = default_edges(dims, cell_size)
    if bins is None and k_range is None:
        if k_log:
            raise ValueError("k_log needs bins or k_range")
        return default
    bins = default.size - 1 if bins is None else int(bins)
    if not 1 <= bins <= MAX_BINS:
        raise ValueError(f"bins must lie in [1, {MAX_BINS}]")
    if k_range is None:
        k_range = (default[1] if k_log else default[0], default[-1])
    lo, hi = (float(v) for v in k_range)
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 <= lo < hi):
        raise ValueError("k_range must be (k_min, k_max) with 0 <= k_min < k_max, both finite")
    if k_log:
        if lo <= 0.0:
            raise ValueError("k_log needs a k_min above 0")
        return np.geomspace(lo, hi, bins + 1)
    return np.linspace(lo, hi, bins + 1)


def check_edges(edges) -> np.ndarray:
    """edges as float64 [n + 1]: finite, from a value >= 0 on, strictly increasing, 1 <= n <=
    2048; ValueError otherwise."""
    e = np.ascontiguousarray(edges, dtype=np.float64)
    if e.ndim != 1 or not 2 <= e.size <= MAX_BINS + 1:
        raise ValueError(f"edges must hold n + 1 values with n in [1, {MAX_BINS}]")
    if not np.isfinite(e).all() or e[0] < 0.0 or not (np.diff(e) > 0.0).all():
        raise ValueError("edges must be finite, not negative and strictly increasing")
    return e


def squared_edges(edges) -> np.ndarray:
    """E[i] = (e[i] / (2 pi))^2 in float64, the divide first: what a mode's q = sum_d m_d^2 / L_d^2
    is compared with.  ValueError if squaring makes two edges equal (or the edges fail
    check_edges)."""
    e = check_edges(edges)
    scaled = e / (2.0 * math.pi)
    squared = scaled * scaled
    if not (np.diff(squared) > 0.0).all():
        raise ValueError("two edges are equal once squared: they lie too close together")
    return squared


def normalise(sums, n_cells: int, edges) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(power, spectrum, k) of the shell sums of |F|^2: power[b] = sums[b] / f64(n_cells)^2 (the
    powers of all modes add up to the field's mean square), spectrum[b] = power[b] / (e[b + 1] -
    e[b]) and k[b] = 0.5 (e[b] + e[b + 1])."""
    e = check_edges(edges)
    sums = np.ascontiguousarray(sums, dtype=np.float64)
    if sums.shape != (e.size - 1,):
        raise ValueError("sums must hold one value per bin")
    cells = float(int(n_cells))
    power = sums / (cells * cells)
    return power, power / (e[1:] - e[:-1]), 0.5 * (e[:-1] + e[1:])


def save_npz(result: Dict, filename: str) -> None:
    """Writes api.power_spectrum's dict as one .npz (numpy.savez): every entry under its key, a
    field's power, spectrum and modes under "fields/" + its name + "/" + the entry."""
    entries = {key: np.asarray(value) for key, value in result.items() if key != "fields"}
    for name, found in result.get("fields", {}).items():
        for entry in _ENTRIES:
            entries[f"{_FIELD}{name}/{entry}"] = np.asarray(found[entry])
    with open(filename, "wb") as out:      # a file object: savez adds no ".npz" of its own
        np.savez(out, **entries)


def load_npz(filename: str) -> Dict:
    """Reads a file save_npz wrote back into a dict of the same shape: arrays stay arrays, level
    and the counts become ints, lo, dims and cell_size tuples."""
    result: Dict = {"fields": {}}
    with np.load(filename) as data:
        for key in data.files:
            if key.startswith(_FIELD):
                name, entry = key[len(_FIELD):].rsplit("/", 1)
                result["fields"].setdefault(name, {})[entry] = data[key]
            else:
                result[key] = data[key]
    for key in ("level", "outside", "nonfinite", "absent"):
        if key in result:
            result[key] = int(result[key])
    for key in ("lo", "dims", "cell_size"):
        if key in result:
            result[key] = tuple(result[key].tolist())
    return result


# ---- Helmholtz split and potential ("Inverse transform, Helmholtz split, potential") --

PARTS = ("solenoidal", "compressive", "total")
_NESTED = ("power", "spectrum", "modes", "solenoidal", "compressive")   # dicts of arrays
_INTS = ("level", "outside", "nonfinite", "absent")
_FLOATS = ("compressive_fraction", "imag_max", "constant", "self_term")
_TUPLES = ("lo", "dims", "cell_size", "padded_dims")


def compressive_fraction(power_solenoidal, power_compressive, edges) -> float:
    """sum(P_c) / (sum(P_c) + sum(P_s)) over the bins above k = 0, those with a lower edge > 0:
    the mean flow, which counts as solenoidal, stays out of the ratio.  NaN without power there."""
    e = check_edges(edges)
    above = e[:-1] > 0.0
    c = float(np.sum(np.asarray(power_compressive, dtype=np.float64)[above]))
    s = float(np.sum(np.asarray(power_solenoidal, dtype=np.float64)[above]))
    return c / (c + s) if c + s != 0.0 else math.nan


def _save_nested(result: Dict, filename: str) -> None:
    entries = {}
    for key, value in result.items():
        if key in _NESTED:
            for name, array in value.items():
                entries[f"{key}/{name}"] = np.asarray(array)
        else:
            entries[key] = np.asarray(value)
    with open(filename, "wb") as out:      # a file object: savez adds no ".npz" of its own
        np.savez(out, **entries)


def _load_nested(filename: str) -> Dict:
    result: Dict = {}
    with np.load(filename) as data:
        for key in data.files:
            head, _, name = key.partition("/")
            if head in _NESTED and name:
                result.setdefault(head, {})[name] = data[key]
            else:
                result[key] = data[key]
    for key in _INTS:
        if key in result:
            result[key] = int(result[key])
    for key in _FLOATS:
        if key in result:
            result[key] = float(result[key])
    for key in _TUPLES:
        if key in result:
            result[key] = tuple(result[key].tolist())
    return result


def save_helmholtz_npz(result: Dict, filename: str) -> None:
    """Writes api.helmholtz's dict as one .npz: every entry under its key, the entries of power,
    spectrum and modes under key + "/" + the part, the grids under "solenoidal/" and
    "compressive/" + the field's name."""
    _save_nested(result, filename)


def load_helmholtz_npz(filename: str) -> Dict:
    """Reads a file save_helmholtz_npz wrote back into a dict of the same shape: arrays stay
    arrays, level and the counts become ints, compressive_fraction and imag_max floats, lo, dims
    and cell_size tuples."""
    return _load_nested(filename)


def save_potential_npz(result: Dict, filename: str) -> None:
    """Writes api.potential's dict as one .npz, every entry under its key."""
    _save_nested(result, filename)


def load_potential_npz(filename: str) -> Dict:
    """Reads a file save_potential_npz wrote back into a dict of the same shape."""
    return _load_nested(filename)


# ---- isolated potential ("Isolated potential") ----------------------------------------

MAX_ISOLATED_LENGTH = 512  # cells per axis of a region: its padded axis is at most MAX_LENGTH


def padded_dims(dims) -> Tuple[int, int, int]:
    """(Px, Py, Pz) of a region of dims = (nx, ny, nz) cells: per axis the smallest power of two
    P >= 2 N - 1, the least that keeps the wrapped images of a zero-padded convolution out of
    the region (1 for N = 1, at most 1024).  ValueError unless every N lies in [1, 512]; the
    message names the axis."""
    out = tuple(int(v) for v in dims)
    if len(out) != 3:
        raise ValueError("dims must hold three values")
    for axis, n in zip("xyz", out):
        if not 1 <= n <= MAX_ISOLATED_LENGTH:
            raise ValueError(f"an isolated potential needs between 1 and {MAX_ISOLATED_LENGTH} "
                             f"cells along every axis, not {n} along {axis}: pass a smaller "
                             "region or a coarser level")
    return tuple(1 << (2 * n - 2).bit_length() for n in out)


def check_isolated_dims(dims) -> Tuple[int, int, int]:
    """dims = (nx, ny, nz) as ints, checked as padded_dims checks them."""
    padded_dims(dims)
    return tuple(int(v) for v in dims)


def save_isolated_potential_npz(result: Dict, filename: str) -> None:
    """Writes api.isolated_potential's dict as one .npz, every entry under its key."""
    _save_nested(result, filename)


def load_isolated_potential_npz(filename: str) -> Dict:
    """Reads a file save_isolated_potential_npz wrote back into a dict of the same shape: level
    and absent ints, imag_max, constant and self_term floats, lo, dims, padded_dims and cell_size
    tuples."""
    return _load_nested(filename)
