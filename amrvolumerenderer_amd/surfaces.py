"""Surfaces ("Isosurface"): what api.isosurface works out on the host from the
triangle soup of csrc/avr_isosurface.hip -- areas, the flux of a vector field, a PLY file.  numpy
only.  A surface is float64 [n, 3, 3]: triangle, vertex, coordinate."""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np


def _soup(vertices) -> np.ndarray:
    soup = np.ascontiguousarray(vertices, dtype=np.float64)
    if soup.ndim != 3 or soup.shape[1:] != (3, 3):
        raise ValueError("a surface is an array [n, 3, 3]: triangle, vertex, coordinate")
    return soup


def area_vectors(vertices) -> np.ndarray:
    """0.5 (v1 - v0) x (v2 - v0) per triangle, float64 [n, 3]."""
    soup = _soup(vertices)
    return 0.5 * np.cross(soup[:, 1] - soup[:, 0], soup[:, 2] - soup[:, 0])


def triangle_areas(vertices) -> np.ndarray:
    """0.5 |(v1 - v0) x (v2 - v0)| per triangle, float64 [n]."""
    vectors = area_vectors(vertices)
    return np.sqrt((vectors * vectors).sum(axis=1))


def surface_flux(surface, fx, fy, fz) -> float:
    """The flux of the vector field F through a surface: math.fsum over the triangles of the mean
    of F at the three vertices dotted with the area vector, which points along the triangles'
    normals.  surface: api.isosurface's dict, or its vertices; fx, fy, fz: the components of F at
    the vertices, arrays [n, 3] (api.isosurface's samples), or one number each for a constant
    field."""
    vertices = surface["vertices"] if isinstance(surface, dict) else surface
    vectors = area_vectors(vertices)
    n = vectors.shape[0]
    terms = np.zeros(n, dtype=np.float64)
    for axis, component in enumerate((fx, fy, fz)):
        at_vertices = np.broadcast_to(np.asarray(component, dtype=np.float64), (n, 3)) \
            if np.ndim(component) == 0 else np.asarray(component, dtype=np.float64)
        if at_vertices.shape != (n, 3):
            raise ValueError("a component of F is a number or an array [n, 3]")
        terms = terms + at_vertices.sum(axis=1) / 3.0 * vectors[:, axis]
    return math.fsum(terms.tolist())


def save_ply(vertices, filename: str, samples: Optional[Dict[str, np.ndarray]] = None) -> None:
    """Writes a surface as a binary little-endian PLY file: a triangle soup of 3 n vertices with
    double x, y, z and one double property per entry of samples (name -> array [n, 3]; a name
    must be a word of letters, digits and underscores), then n faces of three int indices."""
    soup = _soup(vertices)
    n = soup.shape[0]
    samples = dict(samples or {})
    columns = [soup.reshape(3 * n, 3)]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {3 * n}",
              "property double x", "property double y", "property double z"]
    for name, values in samples.items():
        if not name or not all(ch.isalnum() or ch == "_" for ch in name) or name in ("x", "y", "z"):
            raise ValueError(f"{name!r} cannot name a PLY property")
        values = np.asarray(values, dtype=np.float64)
        if values.shape != (n, 3):
            raise ValueError(f"samples[{name!r}] must be an array [n, 3]")
        columns.append(values.reshape(3 * n, 1))
        header.append(f"property double {name}")
    header += [f"element face {n}", "property list uchar int vertex_indices", "end_header"]
    faces = np.zeros(n, dtype=[("count", "u1"), ("index", "<i4", (3,))])
    faces["count"] = 3
    faces["index"] = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    with open(filename, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(np.ascontiguousarray(np.concatenate(columns, axis=1), dtype="<f8").tobytes())
        fh.write(faces.tobytes())


def load_ply(filename: str):
    """Reads a file save_ply wrote: (vertices [n, 3, 3], samples {name: [n, 3]})."""
    with open(filename, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError("not a binary little-endian PLY file")
    n_vertices = int(lines[2].split()[2])
    names = [line.split()[2] for line in lines[3:] if line.startswith("property double ")]
    table = np.frombuffer(data, dtype="<f8", count=n_vertices * len(names), offset=end)
    table = table.reshape(n_vertices, len(names))
    n = n_vertices // 3
    vertices = table[:, :3].reshape(n, 3, 3).copy()
    return vertices, {name: table[:, 3 + q].reshape(n, 3).copy()
                      for q, name in enumerate(names[3:])}
