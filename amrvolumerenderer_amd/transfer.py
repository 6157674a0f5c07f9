"""The host side of ray transfer ("Ray transfer"), in numpy: the argument checks of
api.emission_absorption and api.line_cube, the background rule and the expression of the
line-of-sight velocity.  Nothing here touches the device."""
from __future__ import annotations

import math
import operator
from typing import Optional, Sequence

import numpy as np

from . import cubes


def _name(value, what: str, optional: bool = False) -> None:
    if value is None and optional:
        return
    if not isinstance(value, str) or not value:
        raise ValueError(f"{what} must be a variable name{' or None' if optional else ''}, "
                         f"not {value!r}")


def checked_background(background, n_channels: int):
    """background as float64 [n_channels]: one finite value for every channel, or one per
    channel."""
    b = np.asarray(background, dtype=np.float64)
    if b.ndim == 0:
        b = np.full(n_channels, float(b))
    if b.shape != (n_channels,):
        raise ValueError("background must be one value or one value per channel")
    if not np.isfinite(b).all():
        raise ValueError("background must be finite")
    return b


def apply_background(intensity, tau, background):
    """I[c] + background[c] * exp(-tau[c]): what lies behind the far end of every ray, seen through
    the whole optical depth.  intensity, tau: float64 [nc, ...]; background: one value or [nc]."""
    intensity = np.asarray(intensity, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.float64)
    if intensity.shape != tau.shape or intensity.ndim < 1:
        raise ValueError("intensity and tau must have the same shape [channels, ...]")
    b = checked_background(background, intensity.shape[0])
    b = b.reshape((-1,) + (1,) * (intensity.ndim - 1))
    return intensity + b * np.exp(-tau)


def velocity_names(velocity):
    """velocity as a tuple of one name (a line-of-sight velocity, used as it is) or of three (the
    components of a velocity)."""
    if isinstance(velocity, str):
        velocity = (velocity,)
    try:
        names = tuple(velocity)
    except TypeError:
        names = ()
    if len(names) not in (1, 3):
        raise ValueError("velocity must be one variable name or three")
    for name in names:
        _name(name, "velocity")
    return names


def _field(name: str) -> str:
    return name if name.isidentifier() else f"field({name!r})"


def line_of_sight_expression(normal: Sequence[float], names: Sequence[str]) -> str:
    """The derived-field expression of -(n . v): the velocity along the line of sight, positive for
    gas that recedes from a viewer n points at.  normal: the unit normal; its components enter as
    their repr, which reads back as the same floats.  names: the three components' variables."""
    n = tuple(float(c) for c in normal)
    if len(n) != 3 or len(names) != 3 or not all(math.isfinite(c) for c in n):
        raise ValueError("the line of sight needs a finite normal and three velocity components")
    x, y, z = (f"({c!r}) * {_field(name)}" for c, name in zip(n, names))
    return f"-(({x} + {y}) + {z})"


def line_of_sight_values(normal: Sequence[float], vx, vy, vz):
    """What line_of_sight_expression evaluates to, in numpy float64."""
    n = tuple(float(c) for c in normal)
    vx, vy, vz = (np.asarray(v, dtype=np.float64) for v in (vx, vy, vz))
    return -((n[0] * vx + n[1] * vy) + n[2] * vz)


def _size(value, name: str) -> int:
    try:
        size = operator.index(value)
    except TypeError:
        size = 0
    if isinstance(value, bool) or size <= 0:
        raise ValueError(f"{name} must be a positive integer")
    return size


def validate_emission_absorption_arguments(source, opacity, background=0.0, width: int = 512,
                                           height: int = 512, output: Optional[str] = None):
    """The checks of api.emission_absorption that are its own (the view's are
    api.validate_off_axis_projection_arguments'), before the plotfile is opened.  Returns the
    background as a float."""
    _name(source, "source")
    _name(opacity, "opacity")
    _size(width, "width")
    _size(height, "height")
    if output is not None and (not isinstance(output, str) or not output):
        raise ValueError("output must be a file name")
    return float(checked_background(background, 1)[0])


def validate_line_cube_arguments(source, opacity, velocity, width_field=None, channels: int = 64,
                                 v_range=None, edges=None, background=0.0, width: int = 256,
                                 height: int = 256, output: Optional[str] = None):
    """The checks of api.line_cube that are its own, before the plotfile is opened: the names, the
    channels as api.velocity_cube takes them (cubes.validate_cube_arguments), the background and
    the output.  Returns (velocity names, v_range or None, edges or None, background [nc])."""
    _name(source, "source")
    _name(opacity, "opacity")
    names = velocity_names(velocity)
    _, _, rng, edges = cubes.validate_cube_arguments(
        "z", source, names[0], width_field, channels, v_range, edges, width, height, None, None,
        output)
    n = edges.size - 1 if edges is not None else operator.index(channels)
    return names, rng, edges, checked_background(background, n)
