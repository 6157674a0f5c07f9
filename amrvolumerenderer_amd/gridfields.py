"""Grid fields ("Grid fields"): the registry of named fields that are computed on a
uniform grid of one level -- a potential, a component of a Helmholtz split, a caller's own array
-- and written back onto the AMR cells by api.grid_scene, so that every plotfile-level function of
the api takes them as it takes a stored variable.  The registry and its checks only; the
resolution is api._load_variable_scenes'.  numpy only.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np

INTERPOLATIONS = ("constant", "linear")
BOUNDARIES = ("periodic", "isolated")
PARTS = ("solenoidal", "compressive")
COMPONENTS = {"x": 0, "y": 1, "z": 2}

# name -> {"kind": "potential" | "helmholtz" | "array", ...}: the checked arguments
_registry: Dict[str, dict] = {}


def _check_name(name) -> None:
    """The names every registry refuses, and a name one of the other four holds."""
    from . import clumps, derive, gradient
    if not isinstance(name, str) or not name:
        raise ValueError("a grid field's name must be a non-empty string")
    if derive.is_reserved_name(name):
        raise ValueError(f"{name!r} is a built-in, a function or a histogram weight and cannot "
                         "name a grid field")
    if name in derive.derived_fields():
        raise ValueError(f"{name!r} is a registered derived field")
    if name in gradient.gradient_fields():
        raise ValueError(f"{name!r} is a registered gradient field")
    if name in clumps.clump_fields():
        raise ValueError(f"{name!r} is a registered clump field")
    from . import particles
    if name in particles.particle_fields():
        raise ValueError(f"{name!r} is a registered particle field")


def _check_input(of, what: str) -> str:
    if not isinstance(of, str) or not of:
        raise ValueError(f"{what} must be a non-empty field name")
    return of


def _check_interpolation(interpolation) -> str:
    if interpolation not in INTERPOLATIONS:
        raise ValueError('interpolation must be "constant" or "linear"')
    return interpolation


def _check_region(level, region, left_edge, right_edge) -> dict:
    """level, region and edges as api.covering_grid takes them, as far as they can be checked
    without a plotfile."""
    if level is not None:
        if isinstance(level, bool) or int(level) != level or int(level) < 0:
            raise ValueError("level must be None or a level number")
        level = int(level)
    if region is not None and (left_edge is not None or right_edge is not None):
        raise ValueError("give region or left_edge / right_edge, not both")
    if (left_edge is None) != (right_edge is None):
        raise ValueError("left_edge and right_edge go together")
    if region is not None:
        first, last = (tuple(int(v) for v in corner) for corner in region)
        if len(first) != 3 or len(last) != 3:
            raise ValueError("region must be ((ilo, jlo, klo), (ihi, jhi, khi))")
        if min(last[a] - first[a] + 1 for a in range(3)) < 1:
            raise ValueError("region must hold at least one cell along every axis")
        region = (first, last)
    if left_edge is not None:
        left_edge = tuple(float(v) for v in left_edge)
        right_edge = tuple(float(v) for v in right_edge)
        if len(left_edge) != 3 or len(right_edge) != 3 or \
                not all(math.isfinite(v) for v in left_edge + right_edge):
            raise ValueError("left_edge and right_edge must hold three finite values")
    return {"level": level, "region": region, "left_edge": left_edge, "right_edge": right_edge}


def _check_fill(fill) -> Optional[float]:
    return None if fill is None else float(fill)


def _register(name: str, entry: dict) -> None:
    """Puts the entry in, unless a field it is made of is made of it."""
    from . import derive, gradient
    before = _registry.get(name)
    _registry[name] = entry
    try:
        gradient.check_no_cycle(name, derive.derived_fields(), gradient.gradient_fields())
    except ValueError:
        if before is None:
            del _registry[name]
        else:
            _registry[name] = before
        raise


def add_potential_field(name: str, of: str, constant: float = 1.0, boundary: str = "periodic",
                        level: Optional[int] = None, region=None, left_edge=None,
                        right_edge=None, self_term: float = 0.0, fill: Optional[float] = None,
                        interpolation: str = "linear", outside: float = math.nan) -> None:
    """Registers the grid field `name` = the potential of the field `of` for every plotfile-level
    function of the api: wherever they take a variable name, and inside a derived field's
    expression, `name` now means phi with laplace(phi) = constant * `of` -- api.potential's with
    boundary "periodic", api.isolated_potential's (with its self_term) with "isolated" -- computed
    on the covering grid of `level` (by default the call's finest loaded level) over region or
    left_edge / right_edge (by default the whole domain) and written back onto the AMR cells
    (api.grid_scene): interpolated as `interpolation` says where the cells are finer than the
    grid, wrapped at the region's faces exactly when the boundary is periodic, `outside` where the
    grid does not reach.  `of` is a stored variable or a registered field of any kind; level,
    region, edges and fill as api.potential takes them.  Refused: the names add_field refuses, a
    name another registry holds, wrong arguments, and a cycle through the registries."""
    _check_name(name)
    constant, self_term = float(constant), float(self_term)
    if not math.isfinite(constant):
        raise ValueError("constant must be finite")
    if boundary not in BOUNDARIES:
        raise ValueError('boundary must be "periodic" or "isolated"')
    if not (math.isfinite(self_term) and self_term >= 0.0):
        raise ValueError("self_term must be finite and not negative")
    if boundary == "periodic" and self_term != 0.0:
        raise ValueError("self_term belongs to the isolated boundary")
    _register(name, {"kind": "potential", "of": _check_input(of, "a potential field's input"),
                     "constant": constant, "boundary": boundary, "self_term": self_term,
                     **_check_region(level, region, left_edge, right_edge),
                     "fill": _check_fill(fill),
                     "interpolation": _check_interpolation(interpolation),
                     "periodic": boundary == "periodic", "outside": float(outside)})


def add_helmholtz_field(name: str, velocity, part: str = "solenoidal", component: str = "x",
                        level: Optional[int] = None, region=None, left_edge=None,
                        right_edge=None, fill: Optional[float] = None,
                        interpolation: str = "constant", outside: float = math.nan) -> None:
    """Registers the grid field `name` = one component ("x", "y" or "z") of the solenoidal or the
    compressive part of the velocity field `velocity` (three field names), as api.helmholtz
    computes it on a periodic grid, written back onto the AMR cells (api.grid_scene, wrapped at
    the region's faces).  Fields registered on the same velocity, level, region and fill share one
    forward transform and projection per call.  The other arguments and the refusals as
    add_potential_field has them."""
    _check_name(name)
    names = [velocity] if isinstance(velocity, str) else list(velocity)
    if len(names) != 3:
        raise ValueError("velocity must name three components")
    names = tuple(_check_input(v, "a velocity component") for v in names)
    if part not in PARTS:
        raise ValueError('part must be "solenoidal" or "compressive"')
    if component not in COMPONENTS:
        raise ValueError('component must be "x", "y" or "z"')
    _register(name, {"kind": "helmholtz", "velocity": names, "part": part,
                     "component": COMPONENTS[component],
                     **_check_region(level, region, left_edge, right_edge),
                     "fill": _check_fill(fill),
                     "interpolation": _check_interpolation(interpolation), "periodic": True,
                     "outside": float(outside)})


def add_array_field(name: str, array, level: int, lo=(0, 0, 0), interpolation: str = "constant",
                    periodic: bool = False, outside: float = math.nan) -> None:
    """Registers the grid field `name` = the caller's own grid: array is a numpy or torch float64
    [nz, ny, nx] array of the level-`level` cells from the index lo on (kept, not copied), written
    back onto the AMR cells of whichever plotfile a call names (api.grid_scene).  The refusals as
    add_potential_field has them."""
    _check_name(name)
    if isinstance(level, bool) or int(level) != level or not 0 <= int(level) < 16:
        raise ValueError("level must be a level number in [0, 16)")
    first = tuple(int(v) for v in lo)
    if len(first) != 3:
        raise ValueError("lo must hold three values")
    if not hasattr(array, "shape") or not hasattr(array, "dtype"):
        array = np.asarray(array, dtype=np.float64)
    shape = tuple(int(n) for n in array.shape)
    if len(shape) != 3 or min(shape) < 1 or not str(array.dtype).endswith("float64"):
        raise ValueError("array must be a float64 [nz, ny, nx] array with at least one cell")
    if shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError("the array has 2^31 cells or more")
    _register(name, {"kind": "array", "array": array, "level": int(level), "lo": first,
                     "interpolation": _check_interpolation(interpolation),
                     "periodic": bool(periodic), "outside": float(outside)})


def remove_grid_field(name: str) -> None:
    """Forgets a registered grid field (KeyError if there is none of that name)."""
    del _registry[name]


def grid_fields() -> Dict[str, dict]:
    """name -> the checked arguments of every registered grid field (a copy; "kind" says which
    of the three it is)."""
    return {name: dict(entry) for name, entry in _registry.items()}


def inputs_of(name: str) -> Tuple[str, ...]:
    """The fields the grid field `name` is computed from: none for an array."""
    entry = _registry[name]
    if entry["kind"] == "potential":
        return (entry["of"],)
    if entry["kind"] == "helmholtz":
        return tuple(entry["velocity"])
    return ()
