"""Gradient fields ("Gradient fields"): the registry of named differences of a field
along an axis, and what api.gradient_scene works out on the host before the kernels of
csrc/avr_gradient.hip run.  numpy only.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

AXES = {"x": 0, "y": 1, "z": 2, 0: 0, 1: 1, 2: 2}
# how far a recovered box index may lie from an integer
INDEX_TOLERANCE = 1e-6

_registry: Dict[str, Tuple[str, int]] = {}


def _dependencies(name: str, derived: Dict[str, str], gradients: Dict[str, Tuple[str, int]],
                  clumps: Dict[str, tuple]):
    """The names `name` is made of, one step down: a gradient or clump field's input, a registered
    grid field's inputs (gridfields.py), or the fields a derived field reads once the derived
    fields it names are inlined; () for anything else."""
    from . import derive, gridfields, particles
    if name in gridfields.grid_fields():
        return gridfields.inputs_of(name)
    if name in particles.particle_fields():
        return ()                      # a particle field reads no field: a leaf of the graph
    if name in gradients:
        return (gradients[name][0],)
    if name in clumps:
        return (clumps[name][0],)
    if name in derived:
        text = name if name.isidentifier() else f"field({name!r})"
        return derive.compile_expression(text, derived).fields
    return ()


def check_no_cycle(start: str, derived: Dict[str, str], gradients: Dict[str, Tuple[str, int]],
                   clumps: Optional[Dict[str, tuple]] = None) -> None:
    """ValueError if `start` reaches itself through the registries of derived, gradient and clump
    fields (clumps.py; the registered clump fields if None)."""
    if clumps is None:
        from . import clumps as clump_registry
        clumps = clump_registry.clump_fields()

    def visit(name, path):
        if name in path:
            raise ValueError("registered fields refer to each other in a cycle: "
                             + " -> ".join(path + [name]))
        for inner in _dependencies(name, derived, gradients, clumps):
            visit(inner, path + [name])
    visit(start, [])


def add_gradient_field(name: str, of: str, axis) -> None:
    """Registers the gradient field `name` = d(of) / d(axis) for every plotfile-level function of
    the api: wherever they take a variable name, and inside a derived field's expression, `name`
    now means that difference ("Gradient fields").  `of` is a stored variable, a
    registered derived field or another gradient field (a second derivative); axis is 0, 1, 2 or
    "x", "y", "z".  Refused: the names add_field refuses, a name that is a registered derived field,
    and a cycle through either registry."""
    from . import derive
    if not isinstance(name, str) or not name:
        raise ValueError("a gradient field's name must be a non-empty string")
    if not isinstance(of, str) or not of:
        raise ValueError("a gradient field's input must be a non-empty field name")
    if derive.is_reserved_name(name):
        raise ValueError(f"{name!r} is a built-in, a function or a histogram weight and cannot "
                         "name a gradient field")
    derived = derive.derived_fields()
    if name in derived:
        raise ValueError(f"{name!r} is a registered derived field")
    from . import clumps
    if name in clumps.clump_fields():
        raise ValueError(f"{name!r} is a registered clump field")
    from . import gridfields
    if name in gridfields.grid_fields():
        raise ValueError(f"{name!r} is a registered grid field")
    from . import particles
    if name in particles.particle_fields():
        raise ValueError(f"{name!r} is a registered particle field")
    if isinstance(axis, bool) or axis not in AXES:
        raise ValueError("axis must be 0, 1, 2 or 'x', 'y', 'z'")
    trial = dict(_registry)
    trial[name] = (of, AXES[axis])
    check_no_cycle(name, derived, trial)
    _registry[name] = trial[name]


def remove_gradient_field(name: str) -> None:
    """Forgets a registered gradient field (KeyError if there is none of that name)."""
    del _registry[name]


def gradient_fields() -> Dict[str, Tuple[str, int]]:
    """name -> (input field, axis) of every registered gradient field (a copy)."""
    return dict(_registry)


def box_index_lo(min_corners: Sequence[Sequence[float]], levels: Sequence[int], world_scale: float,
                 prob_lo: Sequence[float], cell_sizes) -> np.ndarray:
    """[n_boxes, 3] int32: the index of every box's first cell in its level's index space, from its
    low corner in scene coordinates: (min_corner / world_scale - prob_lo) / dx of the box's level.
    ValueError if one lies more than 1e-6 from an integer (the corners are not those of a plotfile
    with this prob_lo and these cell sizes) or outside 31 bits."""
    out = np.zeros((len(min_corners), 3), dtype=np.int32)
    for b, (corner, level) in enumerate(zip(min_corners, levels)):
        for a in range(3):
            position = (float(corner[a]) / float(world_scale) - float(prob_lo[a])) / \
                float(cell_sizes[int(level)][a])
            nearest = round(position) if np.isfinite(position) else None
            if nearest is None or abs(position - nearest) > INDEX_TOLERANCE or \
                    abs(nearest) >= 2 ** 31:
                raise ValueError(f"box {b}: its low corner along axis {a} is at index {position!r} "
                                 f"of level {int(level)}, which is not an integer")
            out[b, a] = nearest
    return out
