"""Particle fields ("Particle fields"): the registry of named fields that are made of
particles -- positions and values as plain arrays -- deposited onto the AMR cells by
api.deposit_scene, so that every plotfile-level function of the api takes them as it takes a stored
variable.  The registry and its checks only; the resolution is api._load_variable_scenes'.  numpy
only.
"""
from __future__ import annotations

from typing import Dict

import numpy as np

METHODS = ("ngp", "cic")
QUANTITIES = ("sum", "density")

# name -> {"positions": float64 [n, 3], "values": float64 [n] or None, "method", "quantity"}
_registry: Dict[str, dict] = {}


def check_method(method) -> str:
    if method not in METHODS:
        raise ValueError('method must be "ngp" or "cic"')
    return method


def check_quantity(quantity) -> str:
    if quantity not in QUANTITIES:
        raise ValueError('quantity must be "sum" or "density"')
    return quantity


def _real(array) -> bool:
    kind = str(array.dtype).replace("torch.", "")
    return kind.startswith(("float", "int", "uint", "bfloat"))


def check_arrays(positions, values):
    """positions [n, 3] and values [n] or None as they came (numpy, torch, or anything numpy
    takes), checked: ValueError for a wrong shape or a dtype that is not real."""
    if not hasattr(positions, "shape") or not hasattr(positions, "dtype"):
        positions = np.asarray(positions)
        if positions.size == 0:
            positions = positions.reshape(0, 3).astype(np.float64)
    if values is not None and not (hasattr(values, "shape") and hasattr(values, "dtype")):
        values = np.asarray(values)
        if values.size == 0:
            values = values.astype(np.float64)
    if not _real(positions) or (values is not None and not _real(values)):
        raise ValueError("positions and values must be real numbers")
    shape = tuple(int(n) for n in positions.shape)
    if len(shape) != 2 or shape[1] != 3:
        raise ValueError("positions must be [n, 3]")
    if values is not None and tuple(int(n) for n in values.shape) != (shape[0],):
        raise ValueError("values must hold one value per particle")
    return positions, values


def _copied_float64(array) -> np.ndarray:
    if hasattr(array, "detach"):                       # a torch tensor
        array = array.detach().cpu().numpy()
    return np.array(array, dtype=np.float64, copy=True, order="C")


def _check_name(name) -> None:
    """The names every registry refuses, and a name one of the other four holds."""
    from . import clumps, derive, gradient, gridfields
    if not isinstance(name, str) or not name:
        raise ValueError("a particle field's name must be a non-empty string")
    if derive.is_reserved_name(name):
        raise ValueError(f"{name!r} is a built-in, a function or a histogram weight and cannot "
                         "name a particle field")
    if name in derive.derived_fields():
        raise ValueError(f"{name!r} is a registered derived field")
    if name in gradient.gradient_fields():
        raise ValueError(f"{name!r} is a registered gradient field")
    if name in clumps.clump_fields():
        raise ValueError(f"{name!r} is a registered clump field")
    if name in gridfields.grid_fields():
        raise ValueError(f"{name!r} is a registered grid field")


def add_particle_field(name: str, positions, values=None, method: str = "cic",
                       quantity: str = "density") -> None:
    """Registers the particle field `name` for every plotfile-level function of the api: wherever
    they take a variable name, and inside a derived field's expression, `name` now means the
    particles at positions ([n, 3], the plotfile's physical units) with values ([n], or None for
    1.0 each) deposited onto the cells of whichever plotfile a call names (api.deposit_scene):
    method "ngp" (all of a particle in the cell that holds it) or "cic" (shared among the eight
    cell centres around it), quantity "sum" or "density" (the sum over the cell's volume).  Both
    arrays are copied here, as float64.  A particle field reads no other field.  Refused: the names
    add_field refuses, a name another registry holds, wrong shapes, dtypes that are not real, and
    unknown method or quantity names."""
    _check_name(name)
    check_method(method)
    check_quantity(quantity)
    positions, values = check_arrays(positions, values)
    _registry[name] = {"positions": _copied_float64(positions),
                       "values": None if values is None else _copied_float64(values),
                       "method": method, "quantity": quantity}


def remove_particle_field(name: str) -> None:
    """Forgets a registered particle field (KeyError if there is none of that name)."""
    del _registry[name]


def particle_fields() -> Dict[str, dict]:
    """name -> the checked arguments of every registered particle field (a copy of the table; the
    arrays are the registry's own)."""
    return {name: dict(entry) for name, entry in _registry.items()}
