"""Clumps ("Clumps"): the registry of named clump label fields -- the connected
components of the cells of a field whose value lies in [lower, upper] -- and what api.clumps works
out on the host after the kernels of csrc/avr_clumps.hip ran.  numpy only.
"""
from __future__ import annotations

import math
from typing import Dict, Sequence, Tuple

import numpy as np

# n_clumps * n_levels of one table stays below this (avr_scene_clump_table)
TABLE_MAX_ENTRIES = 1 << 28

_registry: Dict[str, Tuple[str, float, float]] = {}


def check_bounds(lower, upper) -> Tuple[float, float]:
    """(lower, upper) as floats; ValueError for a NaN bound or lower > upper.  Either may be
    infinite."""
    lower, upper = float(lower), float(upper)
    if math.isnan(lower) or math.isnan(upper):
        raise ValueError("a clump bound must not be NaN")
    if lower > upper:
        raise ValueError("lower must not exceed upper")
    return lower, upper


def add_clump_field(name: str, of: str, lower: float = -math.inf, upper: float = math.inf) -> None:
    """Registers the clump field `name` for every plotfile-level function of the api: wherever
    they take a variable name, and inside a derived field's expression, `name` now means the label
    field of `of` over [lower, upper] -- f64(label) in 1..N for a cell whose value v satisfies
    lower <= v <= upper, numbered by each clump's smallest cell ordinal, and 0.0 elsewhere
    ("Clumps").  `of` is a stored variable, a derived field, a gradient field or
    another clump field.  Refused: the names add_field refuses, a name held by the registry of
    derived or of gradient fields, a NaN bound or lower > upper, and a cycle through the three
    registries."""
    from . import derive, gradient
    if not isinstance(name, str) or not name:
        raise ValueError("a clump field's name must be a non-empty string")
    if not isinstance(of, str) or not of:
        raise ValueError("a clump field's input must be a non-empty field name")
    if derive.is_reserved_name(name):
        raise ValueError(f"{name!r} is a built-in, a function or a histogram weight and cannot "
                         "name a clump field")
    derived = derive.derived_fields()
    if name in derived:
        raise ValueError(f"{name!r} is a registered derived field")
    gradients = gradient.gradient_fields()
    if name in gradients:
        raise ValueError(f"{name!r} is a registered gradient field")
    lower, upper = check_bounds(lower, upper)
    trial = dict(_registry)
    trial[name] = (of, lower, upper)
    gradient.check_no_cycle(name, derived, gradients, trial)
    _registry[name] = trial[name]


def remove_clump_field(name: str) -> None:
    """Forgets a registered clump field (KeyError if there is none of that name)."""
    del _registry[name]


def clump_fields() -> Dict[str, Tuple[str, float, float]]:
    """name -> (input field, lower, upper) of every registered clump field (a copy)."""
    return dict(_registry)


def clump_volumes(cells_by_level, cell_volumes: Sequence[float]) -> np.ndarray:
    """sum_l vol[l] * f64(cells[l]) per clump, float64, level ascending from +0.0."""
    cells = np.asarray(cells_by_level)
    values = np.zeros(cells.shape[1:], dtype=np.float64)
    for level in range(cells.shape[0]):
        values = values + np.float64(cell_volumes[level]) * cells[level].astype(np.float64)
    return values


def clump_integrals(sums_by_level, cell_volumes: Sequence[float]) -> np.ndarray:
    """sum_l vol[l] * sums[l] per clump, float64, level ascending from +0.0: the volume integral of
    the summed field over each clump."""
    sums = np.asarray(sums_by_level, dtype=np.float64)
    values = np.zeros(sums.shape[1:], dtype=np.float64)
    for level in range(sums.shape[0]):
        values = values + np.float64(cell_volumes[level]) * sums[level]
    return values
