"""Lines ("Streamlines"): what api.streamlines works out on the host from the points of
csrc/avr_streamlines.hip -- the join of a backward and a forward line, lengths, a legacy-VTK file.
numpy only; no device work."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np


def split_lines(points, counts) -> List[np.ndarray]:
    """points [n, m, 3] and counts [n] -> the list of [count_i, 3] arrays (copies)."""
    points = np.asarray(points, dtype=np.float64)
    return [points[i, :int(c)].copy() for i, c in enumerate(np.asarray(counts).tolist())]


def join_both(backward: Sequence[np.ndarray], forward: Sequence[np.ndarray]) -> List[np.ndarray]:
    """Per seed the backward line reversed, then the forward line, the seed kept once.  Both lines
    of a seed start at the seed, or both are empty (the seed is outside).  Works on [count, 3]
    points and on [count] sample values alike."""
    if len(backward) != len(forward):
        raise ValueError("the backward and the forward lines must come from the same seeds")
    return [np.concatenate([np.asarray(b)[:0:-1], np.asarray(f)]) for b, f in zip(backward, forward)]


def line_lengths(lines: Sequence[np.ndarray]) -> np.ndarray:
    """Per line the math.fsum of its segments' lengths sqrt((dx dx + dy dy) + dz dz)."""
    out = np.zeros(len(lines), dtype=np.float64)
    for i, line in enumerate(lines):
        d = np.diff(np.asarray(line, dtype=np.float64).reshape(-1, 3), axis=0)
        out[i] = math.fsum(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).tolist())
    return out


def _checked(lines, samples):
    lines = [np.ascontiguousarray(line, dtype=np.float64) for line in lines]
    for line in lines:
        if line.ndim != 2 or line.shape[1] != 3:
            raise ValueError("a line must be an array [count, 3]")
    checked = {}
    for name, values in (samples or {}).items():
        name = str(name)
        if not name or any(c.isspace() for c in name):
            raise ValueError("a sample's name must be one word")
        values = [np.ascontiguousarray(v, dtype=np.float64) for v in values]
        if len(values) != len(lines) or any(v.shape != (line.shape[0],)
                                            for v, line in zip(values, lines)):
            raise ValueError("a sample must hold one value per point of every line")
        checked[name] = values
    return lines, checked


def save_vtk_lines(lines: Sequence[np.ndarray], filename: str,
                   samples: Optional[Dict[str, Sequence[np.ndarray]]] = None) -> None:
    """Writes lines (a list of [count_i, 3] arrays) as a legacy-VTK ASCII POLYDATA file: POINTS,
    one LINES cell per line (an empty line is a cell of no points) and, per entry of samples
    {name: list of [count_i]}, one SCALARS array of POINT_DATA.  Numbers are written with repr, so
    load_vtk_lines gives back equal bits."""
    lines, samples = _checked(lines, samples)
    total = sum(line.shape[0] for line in lines)
    with open(filename, "w") as out:
        out.write("# vtk DataFile Version 3.0\nstreamlines\nASCII\nDATASET POLYDATA\n")
        out.write(f"POINTS {total} double\n")
        for line in lines:
            for x, y, z in line.tolist():
                out.write(f"{x!r} {y!r} {z!r}\n")
        out.write(f"LINES {len(lines)} {len(lines) + total}\n")
        first = 0
        for line in lines:
            n = line.shape[0]
            out.write(" ".join([str(n)] + [str(first + i) for i in range(n)]) + "\n")
            first += n
        if samples:
            out.write(f"POINT_DATA {total}\n")
            for name, values in samples.items():
                out.write(f"SCALARS {name} double 1\nLOOKUP_TABLE default\n")
                for per_line in values:
                    for v in per_line.tolist():
                        out.write(f"{v!r}\n")


def load_vtk_lines(filename: str) -> Tuple[List[np.ndarray], Dict[str, List[np.ndarray]]]:
    """Reads a file save_vtk_lines wrote: (lines, samples)."""
    with open(filename) as fh:
        header = [fh.readline() for _ in range(4)]
        if not header[0].startswith("# vtk DataFile") or header[2].strip() != "ASCII" or \
                header[3].split() != ["DATASET", "POLYDATA"]:
            raise ValueError(f"{filename} is not a legacy-VTK ASCII POLYDATA file")
        words = fh.read().split()
    at = 0

    def take(n):
        nonlocal at
        if at + n > len(words):
            raise ValueError(f"{filename} ends early")
        at += n
        return words[at - n:at]

    key, total, kind = take(3)
    if key != "POINTS" or kind != "double":
        raise ValueError(f"{filename}: expected POINTS of doubles")
    total = int(total)
    points = np.array([float(w) for w in take(3 * total)], dtype=np.float64).reshape(total, 3)
    key, n_lines, size = take(3)
    if key != "LINES":
        raise ValueError(f"{filename}: expected LINES")
    lines, cells_end = [], at + int(size)
    for _ in range(int(n_lines)):
        n = int(take(1)[0])
        index = [int(w) for w in take(n)]
        lines.append(points[index].reshape(n, 3))
    if at != cells_end:
        raise ValueError(f"{filename}: the LINES section has another size than it says")
    samples: Dict[str, List[np.ndarray]] = {}
    if at < len(words):
        key, count = take(2)
        if key != "POINT_DATA" or int(count) != total:
            raise ValueError(f"{filename}: expected POINT_DATA for every point")
        while at < len(words):
            key, name, kind, _ = take(4)
            if key != "SCALARS" or kind != "double" or take(2) != ["LOOKUP_TABLE", "default"]:
                raise ValueError(f"{filename}: expected SCALARS of doubles")
            values = np.array([float(w) for w in take(total)], dtype=np.float64)
            ends = np.cumsum([line.shape[0] for line in lines]).tolist()
            samples[name] = [values[e - line.shape[0]:e] for e, line in zip(ends, lines)]
    return lines, samples
