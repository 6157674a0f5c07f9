"""Clumps ("Clumps"): the registry of named clump label fields -- the connected
components of the cells of a field whose value lies in [lower, upper] -- and what api.clumps works
out on the host after the kernels of csrc/avr_clumps.hip ran; and the host side of the clump tree
("Clump tree"): the ladder's rules, the node numbering, yt's collapse and the .npz
writer.  numpy only.
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
    from . import gridfields
    if name in gridfields.grid_fields():
        raise ValueError(f"{name!r} is a registered grid field")
    from . import particles
    if name in particles.particle_fields():
        raise ValueError(f"{name!r} is a registered particle field")
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


# ---- clump trees ("Clump tree") -----------------------------------------------------

LADDER_MAX_THRESHOLDS = 64


def check_thresholds(thresholds, upper=math.inf) -> Tuple[Tuple[float, ...], float]:
    """(thresholds, upper) as floats: 1 to 64 finite values, strictly ascending, under one closed
    upper bound that may be +inf, is no NaN and is not below the last threshold; ValueError
    otherwise."""
    values = tuple(float(t) for t in thresholds)
    upper = float(upper)
    if not 1 <= len(values) <= LADDER_MAX_THRESHOLDS:
        raise ValueError("a ladder holds 1 to 64 thresholds")
    if not all(math.isfinite(t) for t in values):
        raise ValueError("thresholds must be finite")
    if any(b <= a for a, b in zip(values, values[1:])):
        raise ValueError("thresholds must be strictly ascending")
    if math.isnan(upper):
        raise ValueError("a clump bound must not be NaN")
    if values[-1] > upper:
        raise ValueError("the last threshold must not exceed upper")
    return values, upper


def threshold_ladder(c_min: float, c_max: float, step: float) -> np.ndarray:
    """yt's ladder: t[0] = c_min, t[i + 1] = t[i] * step (one f64 multiply), every value <= c_max
    kept.  Needs step > 1, 0 < c_min <= c_max, all finite, and at most 64 values: anything else is
    a ValueError."""
    c_min, c_max, step = float(c_min), float(c_max), float(step)
    if not (math.isfinite(c_min) and math.isfinite(c_max) and math.isfinite(step)):
        raise ValueError("c_min, c_max and step must be finite")
    if not step > 1.0:
        raise ValueError("step must exceed 1")
    if not 0.0 < c_min <= c_max:
        raise ValueError("0 < c_min <= c_max is required")
    values = [c_min]
    while True:
        following = float(np.float64(values[-1]) * np.float64(step))
        if not following <= c_max:
            break
        if len(values) == LADDER_MAX_THRESHOLDS:
            raise ValueError("the ladder holds more than 64 thresholds")
        values.append(following)
    return np.array(values, dtype=np.float64)


def tree_nodes(counts: Sequence[int], parents_per_threshold) -> Dict[str, np.ndarray]:
    """The nodes of a clump tree.  counts[i]: the number of clumps of threshold i;
    parents_per_threshold[i] (i >= 1): per clump of threshold i, ascending label, the label
    (1-based) of the clump of threshold i - 1 that holds it; entry 0 is not read.  Nodes are
    numbered by ascending threshold, then label.  Returns node_begin int64 [k + 1],
    threshold_index, label, parent (node id, -1 at threshold 0) int64 [n], and the children as
    CSR: child_offsets int64 [n + 1], children int64 (ascending per node)."""
    counts = [int(c) for c in counts]
    if any(c < 0 for c in counts):
        raise ValueError("a count is negative")
    node_begin = np.zeros(len(counts) + 1, dtype=np.int64)
    node_begin[1:] = np.cumsum(np.array(counts, dtype=np.int64))
    n = int(node_begin[-1])
    threshold_index = np.repeat(np.arange(len(counts), dtype=np.int64),
                                np.array(counts, dtype=np.int64))
    label = np.concatenate([np.arange(1, c + 1, dtype=np.int64) for c in counts] +
                           [np.zeros(0, dtype=np.int64)])
    parent = np.full(n, -1, dtype=np.int64)
    for i in range(1, len(counts)):
        held_by = np.asarray(parents_per_threshold[i], dtype=np.int64).reshape(-1)
        if held_by.size != counts[i]:
            raise ValueError("parents_per_threshold must hold one label per clump")
        if counts[i] and (held_by.min() < 1 or held_by.max() > counts[i - 1]):
            raise ValueError("a parent label is no clump of the threshold below")
        parent[node_begin[i]:node_begin[i + 1]] = node_begin[i - 1] + held_by - 1
    has_parent = parent >= 0
    child_offsets = np.zeros(n + 1, dtype=np.int64)
    child_offsets[1:] = np.cumsum(np.bincount(parent[has_parent], minlength=n))
    nodes = np.nonzero(has_parent)[0].astype(np.int64)
    children = nodes[np.argsort(parent[has_parent], kind="stable")]
    return {"node_begin": node_begin, "threshold_index": threshold_index, "label": label,
            "parent": parent, "child_offsets": child_offsets, "children": children}


def collapse_tree(parent, cells, min_cells: int = 1, passes=None) -> Dict[str, np.ndarray]:
    """yt's rule that a clump which does not split is the same clump, on a finished tree (parent:
    node ids, -1 for a root, every parent before its children; cells per node).  valid[v] =
    cells[v] >= min_cells and passes[v] and (v is a root or valid[parent[v]]) -- passes: one
    bool per node, a further validator's verdict such as bound_mask's, all true by default;
    validity is inherited from the top down, as yt never looks below a child it rejected.  Without
    passes this is cells[v] >= min_cells alone, a child holding no more cells than its parent.
    kept[v] = valid[v] and (v is a root or its parent has at least two
    valid children); kept_parent[v] = for a kept v the first kept node met walking up from
    parent[v] (-1 for a root), for any other node -1; leaves = the kept nodes that are no kept
    node's kept_parent, ascending.  Returns kept bool [n], kept_parent int64 [n], leaves int64."""
    parent = np.asarray(parent, dtype=np.int64).reshape(-1)
    cells = np.asarray(cells, dtype=np.int64).reshape(-1)
    if parent.shape != cells.shape:
        raise ValueError("parent and cells must hold one entry per node")
    n = parent.size
    valid = cells >= int(min_cells)
    if passes is not None:
        passes = np.asarray(passes, dtype=bool).reshape(-1)
        if passes.shape != parent.shape:
            raise ValueError("passes must hold one entry per node")
        valid = valid & passes
        for v in range(n):      # every parent before its children
            if parent[v] >= 0 and not valid[parent[v]]:
                valid[v] = False
    below = valid & (parent >= 0)
    valid_children = np.bincount(parent[below], minlength=n) if n else np.zeros(0, dtype=np.int64)
    kept = valid & ((parent < 0) | (valid_children[np.maximum(parent, 0)] >= 2))
    kept_parent = np.full(n, -1, dtype=np.int64)
    for v in range(n):
        if not kept[v]:
            continue
        up = int(parent[v])
        while up >= 0 and not kept[up]:
            up = int(parent[up])
        kept_parent[v] = up
    is_parent = np.zeros(n, dtype=bool)
    is_parent[kept_parent[kept_parent >= 0]] = True
    leaves = np.nonzero(kept & ~is_parent)[0].astype(np.int64)
    return {"kept": kept, "kept_parent": kept_parent, "leaves": leaves}


# ---- clump binding ("Clump binding") ------------------------------------------------

BINDING_MAX_CELLS = 1 << 22        # members of one evaluated clump (avr_clump_pair_energy)
BINDING_MAX_MEMBERS = 1 << 31      # members of one call stay below this
BINDING_DEFAULT_MAX_CELLS = 1 << 18     # a guess: tools/clump_binding_timing.py measures it


def member_segments(cells, min_cells: int = 1, max_cells: int = BINDING_DEFAULT_MAX_CELLS):
    """Which clumps' cells are listed and where they lie in the member list.  cells: the cell
    count per clump, label ascending.  wanted[c] = min_cells <= cells[c] <= max_cells; offsets:
    the prefix sum of the wanted clumps' counts in label order, from 0.  ValueError for 2^31
    members or more.  Returns (wanted bool [n], offsets int64 [wanted.sum() + 1])."""
    cells = np.asarray(cells, dtype=np.int64).reshape(-1)
    wanted = (cells >= int(min_cells)) & (cells <= int(max_cells))
    offsets = np.zeros(int(wanted.sum()) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(cells[wanted])
    if int(offsets[-1]) >= BINDING_MAX_MEMBERS:
        raise ValueError("the wanted clumps hold 2^31 cells or more")
    return wanted, offsets


def check_max_cells(max_cells) -> int:
    """max_cells as an int; ValueError above 2^22, the most one segment of avr_clump_pair_energy
    holds."""
    if int(max_cells) > BINDING_MAX_CELLS:
        raise ValueError("max_cells must not exceed 2^22")
    return int(max_cells)


def binding_segments(cells, min_cells: int = 1, max_cells: int = BINDING_DEFAULT_MAX_CELLS):
    """Which clumps are evaluated for binding: member_segments over max(min_cells, 2) <= cells[c]
    <= max_cells -- a clump of one cell has no pair.  ValueError for max_cells above 2^22
    (check_max_cells)."""
    return member_segments(cells, max(int(min_cells), 2), check_max_cells(max_cells))


def pair_energy(x, y, z, m, offsets) -> np.ndarray:
    """The numpy twin of avr_clump_pair_energy: per segment sum_{i<j} m_i m_j / r_ij with r_ij =
    sqrt((dx dx + dy dy) + dz dz) in float64, the terms of member i against every j > i made
    row-wise by numpy -- the same correctly rounded operations as the kernel's.  math.fsum adds a
    row's terms exactly and rounds once, and then the rows' sums in the same way: two roundings,
    so within 2 * 2^-53 of the exact sum of the terms, which are not negative.  +0.0 for fewer
    than two members."""
    x, y, z, m = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (x, y, z, m))
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    energy = np.zeros(max(offsets.size - 1, 0), dtype=np.float64)
    for s in range(energy.size):
        lo, hi = int(offsets[s]), int(offsets[s + 1])
        rows = []
        for i in range(lo, hi - 1):
            dx, dy, dz = x[i] - x[i + 1:hi], y[i] - y[i + 1:hi], z[i] - z[i + 1:hi]
            with np.errstate(divide="ignore", invalid="ignore"):
                terms = m[i] * m[i + 1:hi] / np.sqrt((dx * dx + dy * dy) + dz * dz)
            rows.append(math.fsum(terms.tolist()))
        energy[s] = math.fsum(rows)
    return energy


def bound_mask(G: float, W, K, T, evaluated) -> np.ndarray:
    """yt's gravitationally_bound per clump: G * W > K + T where the clump was evaluated, True
    where it was not -- an envelope too large to sum is kept."""
    W, K, T = (np.asarray(a, dtype=np.float64) for a in (W, K, T))
    evaluated = np.asarray(evaluated, dtype=bool)
    with np.errstate(invalid="ignore"):
        return np.where(evaluated, np.float64(G) * W > K + T, True)


def save_tree_npz(path: str, tree: dict) -> None:
    """Writes the dict api.clump_tree returns as one .npz: every array under its key, the
    integrals as integral_<name>, the scalars as zero-dimensional arrays."""
    arrays = {}
    for key, value in tree.items():
        if key == "integrals":
            for name, values in value.items():
                arrays[f"integral_{name}"] = np.asarray(values)
        else:
            arrays[key] = np.asarray(value)
    np.savez(path, **arrays)
