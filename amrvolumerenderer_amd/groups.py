"""Particle groups ("Particle groups"): what api.particle_groups does on the host -- the
checks that come before any device work, the choice of the cell grid, and the catalogue of the
groups (members, mass, centre, velocity, dispersion) from the labels.  numpy only; the grouping
itself is the device's (csrc/avr_particle_groups.hip).
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import numpy as np

from .particles import _real

# What the link kernel finishes in about ten seconds on an MI355X: tools/particle_group_timing.py
# measured 2.4e11 pair tests a second where the cells are full ("Particle groups",
# "Measured"), and 2^41 = 2.2e12.
DEFAULT_MAX_PAIR_TESTS = 2 ** 41
MAX_DIM = 1024              # cells along an axis (the native plan's bound)
MAX_CELLS = 2 ** 27 - 1     # cells in all (the native plan's bound)
_SLACK = 1.0009765625       # 1 + 2^-10: a cell is at least this many linking lengths wide


def linking_length(n: int, volume: float, b: float = 0.2) -> float:
    """The conventional linking length: b times the mean particle separation (volume / n) ** (1/3)."""
    n, volume, b = int(n), float(volume), float(b)
    if n < 1 or not (math.isfinite(volume) and volume > 0.0) or not (math.isfinite(b) and b > 0.0):
        raise ValueError("linking_length needs n >= 1, a finite positive volume and a finite "
                         "positive b")
    return b * (volume / n) ** (1.0 / 3.0)


def _as_numpy(array) -> np.ndarray:
    if hasattr(array, "detach"):                       # a torch tensor
        array = array.detach().cpu().numpy()
    return np.ascontiguousarray(array, dtype=np.float64)


def check_arguments(positions, linking_length_, masses, velocities, min_members, domain, periodic,
                    max_pair_tests):
    """Everything api.particle_groups refuses before any device work, as ValueError.  Returns
    (positions float64 [n, 3], masses float64 [n] or None, velocities float64 [n, 3] or None,
    b, min_members, box or None, flags (three bools), cap or None); the box is (lo, hi) as float64
    [3] arrays, or the plotfile's prob_lo and prob_hi where domain is a path."""
    if not hasattr(positions, "shape") or not hasattr(positions, "dtype"):
        positions = np.asarray(positions)
        if positions.size == 0:
            positions = positions.reshape(0, 3).astype(np.float64)
    for name, array in (("masses", masses), ("velocities", velocities)):
        if array is not None and not (hasattr(array, "shape") and hasattr(array, "dtype")):
            array = np.asarray(array)
            if array.size == 0:
                array = array.astype(np.float64)
            if name == "masses":
                masses = array
            else:
                velocities = array
    for array in (positions, masses, velocities):
        if array is not None and not _real(array):
            raise ValueError("positions, masses and velocities must be real numbers")
    shape = tuple(int(v) for v in positions.shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError("positions must be [n, 3]")
    n = shape[0]
    if n >= 2 ** 31:
        raise ValueError("n must stay below 2^31")
    if masses is not None and tuple(int(v) for v in masses.shape) != (n,):
        raise ValueError("masses must hold one value per particle")
    if velocities is not None and tuple(int(v) for v in velocities.shape) != (n, 3):
        raise ValueError("velocities must be [n, 3]")
    try:
        b = float(linking_length_)
    except (TypeError, ValueError):
        raise ValueError("linking_length must be a finite positive number") from None
    if not (math.isfinite(b) and b > 0.0):
        raise ValueError("linking_length must be a finite positive number")
    if isinstance(min_members, bool) or int(min_members) != min_members or \
            not 1 <= int(min_members) < 2 ** 31:
        raise ValueError("min_members must be an integer in [1, 2^31)")
    try:
        flags = tuple(bool(v) for v in np.broadcast_to(np.asarray(periodic, dtype=bool), (3,)))
    except ValueError:
        raise ValueError("periodic must be a flag or three") from None
    box = None
    if domain is None:
        if any(flags):
            raise ValueError("periodic needs a domain: the period is the domain's extent")
    else:
        if isinstance(domain, (str, bytes)) or hasattr(domain, "__fspath__"):
            from . import plotfile
            header = plotfile.PlotFileData(str(domain))
            domain = (header.prob_lo, header.prob_hi)
        try:
            lo, hi = (np.array(v, dtype=np.float64) for v in domain)
        except (TypeError, ValueError):
            raise ValueError("domain must be (lo, hi), three values each, or a plotfile") from None
        if lo.shape != (3,) or hi.shape != (3,):
            raise ValueError("domain must be (lo, hi), three values each, or a plotfile")
        if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (lo < hi).all()):
            raise ValueError("domain must be finite with lo < hi")
        box = (lo, hi)
        for d in range(3):
            if flags[d] and (hi[d] - lo[d]) / 3.0 < b * _SLACK:
                raise ValueError("linking_length must stay below a third of the period")
    cap = None
    if max_pair_tests is not None:
        if isinstance(max_pair_tests, bool) or int(max_pair_tests) != max_pair_tests or \
                int(max_pair_tests) < 0:
            raise ValueError("max_pair_tests must be a non-negative integer")
        cap = int(max_pair_tests)
    return (positions, masses, velocities, b, int(min_members), box, flags, cap)


def bounding_box(finite_lo, finite_hi, b: float) -> Tuple[np.ndarray, np.ndarray]:
    """The box of a call without a domain from the per-axis minimum and maximum of the finite
    coordinates (None where there is none): an axis without extent gets one linking length."""
    lo, hi = np.zeros(3), np.zeros(3)
    for d in range(3):
        if finite_lo[d] is not None:
            lo[d], hi[d] = float(finite_lo[d]), float(finite_hi[d])
        if not hi[d] > lo[d] or not math.isfinite(hi[d] - lo[d]):
            hi[d] = lo[d] + max(b, abs(lo[d]) * 2.0 ** -40)
            if not hi[d] > lo[d] or not math.isfinite(hi[d]):
                raise ValueError("the positions' bounding box is not finite")
    return lo, hi


def choose_dims(n: int, b: float, lo, hi, flags) -> Tuple[int, int, int]:
    """The cell grid of a call: along every axis as many cells as the rule h >= b (1 + 2^-10)
    admits, at most 1024, then coarsened evenly until there are about 4 n cells at most (and fewer
    than 2^27); a periodic axis keeps at least 3.  The groups do not depend on it."""
    least = [3 if f else 1 for f in flags]
    dims = []
    for d in range(3):
        length = float(hi[d]) - float(lo[d])
        m = int(min(float(MAX_DIM), max(1.0, math.floor(length / (b * _SLACK)))))
        while m > 1 and length / m < b * _SLACK:      # the rule as the native plan evaluates it
            m -= 1
        if m < least[d]:
            raise ValueError("linking_length must stay below a third of the period")
        dims.append(m)
    cap = min(MAX_CELLS, max(4 * int(n), 27))
    product = dims[0] * dims[1] * dims[2]
    if product > cap:
        factor = (cap / product) ** (1.0 / 3.0)
        dims = [max(least[d], int(dims[d] * factor)) for d in range(3)]
    while dims[0] * dims[1] * dims[2] > cap:
        d = max(range(3), key=lambda a: dims[a] - least[a])
        if dims[d] == least[d]:
            break
        dims[d] -= 1
    return tuple(dims)


def member_lists(labels: np.ndarray, count: int):
    """(offsets int64 [count + 1], members int64: particle indices by label, then ascending index,
    first int64 [count]: each group's smallest member, its root)."""
    labels = np.asarray(labels)
    order = np.argsort(labels, kind="stable")
    members = order[np.searchsorted(labels[order], 1):].astype(np.int64)
    sizes = np.bincount(labels[members], minlength=count + 1)[1:count + 1]
    offsets = np.zeros(count + 1, dtype=np.int64)
    np.cumsum(sizes, out=offsets[1:])
    first = members[offsets[:-1]] if count else np.zeros(0, dtype=np.int64)
    return offsets, members, first


def _segment_sums(terms: np.ndarray, offsets: np.ndarray) -> np.ndarray:
    """The sum of terms[offsets[g] : offsets[g + 1]] per group g; every group has a member."""
    if offsets.size <= 1:
        return np.zeros((0,) + terms.shape[1:])
    return np.add.reduceat(terms, offsets[:-1], axis=0)


def catalogue(positions: np.ndarray, masses: Optional[np.ndarray],
              velocities: Optional[np.ndarray], offsets: np.ndarray, members: np.ndarray,
              lo, hi, flags) -> dict:
    """mass [count], centre [count, 3] and, with velocities, velocity [count, 3] and dispersion
    [count] of the groups, as float64 sums over the member-ordered arrays (np.add.reduceat):
    mass = sum m; centre = sum(m x) / mass, on a periodic axis the first member's coordinate x0
    plus sum(m d) / mass over the minimum-image offsets d = x - x0 (d - L above L / 2, d + L below
    -L / 2), wrapped into [lo, hi); velocity = sum(m v) / mass; dispersion = sqrt(sum(m ((dvx dvx +
    dvy dvy) + dvz dvz)) / (3 mass)) with dv = v - velocity.  A group wider than half the period has
    no meaningful centre."""
    count = int(offsets.size) - 1
    x = positions[members]
    m = np.ones(members.size) if masses is None else masses[members]
    mass = _segment_sums(m, offsets)
    sizes = np.diff(offsets)
    centre = np.zeros((count, 3))
    for d in range(3):
        if flags[d]:
            length = float(hi[d]) - float(lo[d])
            x0 = np.repeat(x[offsets[:-1], d], sizes)
            off = x[:, d] - x0
            off = np.where(off > 0.5 * length, off - length, off)
            off = np.where(off < -0.5 * length, off + length, off)
            c = x[offsets[:-1], d] + _segment_sums(m * off, offsets) / mass
            c = np.where(c < lo[d], c + length, c)
            c = np.where(c >= hi[d], c - length, c)
            centre[:, d] = c
        else:
            centre[:, d] = _segment_sums(m * x[:, d], offsets) / mass
    out = {"mass": mass, "centre": centre}
    if velocities is not None:
        v = velocities[members]
        mean = _segment_sums(m[:, None] * v, offsets) / mass[:, None]
        dv = v - np.repeat(mean, sizes, axis=0)
        spread = m * ((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
        out["velocity"] = mean
        out["dispersion"] = np.sqrt(_segment_sums(spread, offsets) / (3.0 * mass))
    return out
