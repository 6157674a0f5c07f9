"""The numpy reference of the particle groups ("Particle groups"): friends-of-friends by
all pairs, in row chunks, with a Python union-find.  There is no grid anywhere in it: what is
outside, which pairs are linked and how the groups are numbered follow the definition alone, with
the link test's operations in the definition's order (numpy's float64 +, -, * are IEEE and nothing
is fused)."""
import math

import numpy as np

CHUNK = 512


def box_of(lo, hi, periodic=False):
    lo = np.array(lo, dtype=np.float64)
    hi = np.array(hi, dtype=np.float64)
    flags = np.broadcast_to(np.asarray(periodic, dtype=bool), (3,)).copy()
    return lo, hi, flags


def inside_of(points, lo, hi, flags):
    """Every coordinate finite and, on a periodic axis, in [lo, hi)."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    inside = np.isfinite(points).all(axis=1)
    for d in range(3):
        if flags[d]:
            with np.errstate(invalid="ignore"):
                inside &= (points[:, d] >= lo[d]) & (points[:, d] < hi[d])
    return inside


def linked(points, rows, b, lo, hi, flags):
    """[len(rows), n] bool: d2 <= b2 with b2 = b * b, d2 = (dx dx + dy dy) + dz dz, per axis a =
    |x_q - x_p| and on a periodic axis a = min(a, L - a) with L = hi - lo.  Only rows and columns of
    inside particles mean anything."""
    b2 = np.float64(b) * np.float64(b)
    with np.errstate(invalid="ignore", over="ignore"):
        a = []
        for d in range(3):
            s = np.abs(points[None, :, d] - points[rows, d][:, None])
            if flags[d]:
                length = hi[d] - lo[d]
                other = length - s
                s = np.where(other < s, other, s)
            a.append(s)
        d2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
        return d2 <= b2


def groups(points, b, lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0), periodic=False, min_members=1):
    """{"labels" int32 [n], "count", "first" int64 [count], "offsets", "members", "sizes" int64
    [count], "outside", "root" int64 [n] (-1 outside)}."""
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = points.shape[0]
    lo, hi, flags = box_of(lo, hi, periodic)
    inside = inside_of(points, lo, hi, flags)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for start in range(0, n, CHUNK):
        rows = np.arange(start, min(start + CHUNK, n))
        hit = linked(points, rows, b, lo, hi, flags)
        hit &= inside[None, :] & inside[rows][:, None]
        hit &= np.arange(n)[None, :] > rows[:, None]
        for r, q in zip(*np.nonzero(hit)):
            u, v = find(int(rows[r])), find(int(q))
            if u != v:
                parent[max(u, v)] = min(u, v)      # the root is the smallest index
    root = np.array([find(p) if inside[p] else -1 for p in range(n)], dtype=np.int64)
    sizes = np.bincount(root[inside], minlength=n) if n else np.zeros(0, dtype=np.int64)
    labels = np.zeros(n, dtype=np.int32)
    first = [r for r in range(n) if inside[r] and root[r] == r and sizes[r] >= min_members]
    number = {r: g + 1 for g, r in enumerate(first)}
    for p in range(n):
        if inside[p] and int(root[p]) in number:
            labels[p] = number[int(root[p])]
    members = [p for g in range(1, len(first) + 1) for p in np.nonzero(labels == g)[0]]
    offsets = np.zeros(len(first) + 1, dtype=np.int64)
    for g, r in enumerate(first):
        offsets[g + 1] = offsets[g] + sizes[r]
    return {"labels": labels, "count": len(first), "first": np.array(first, dtype=np.int64),
            "offsets": offsets, "members": np.array(members, dtype=np.int64),
            "sizes": np.array([sizes[r] for r in first], dtype=np.int64),
            "outside": int(n - inside.sum()), "root": root}


def cell_of(points, lo, hi, dims):
    """The definition's cell index along every axis ([n, 3], int64): floor((x - lo) / h) with h =
    (hi - lo) / dims, clamped to [0, dims - 1].  Finite points only."""
    lo, hi, _ = box_of(lo, hi)
    dims = np.asarray(dims, dtype=np.int64)
    h = (hi - lo) / dims.astype(np.float64)
    q = np.floor((np.asarray(points, dtype=np.float64) - lo) / h)
    return np.clip(q, 0.0, (dims - 1).astype(np.float64)).astype(np.int64)


def pair_tests(points, lo, hi, dims, periodic=False):
    """The unordered pairs of inside particles in the same or in adjacent cells (wrapped on a
    periodic axis), counted pair by pair."""
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    lo, hi, flags = box_of(lo, hi, periodic)
    inside = inside_of(points, lo, hi, flags)
    cells = cell_of(points[inside], lo, hi, dims)
    dims = np.asarray(dims, dtype=np.int64)
    total = 0
    for start in range(0, cells.shape[0], CHUNK):
        rows = cells[start:start + CHUNK]
        near = np.ones((rows.shape[0], cells.shape[0]), dtype=bool)
        for d in range(3):
            gap = np.abs(cells[None, :, d] - rows[:, d][:, None])
            if flags[d]:
                gap = np.minimum(gap, dims[d] - gap)
            near &= gap <= 1
        near &= np.arange(cells.shape[0])[None, :] > (start + np.arange(rows.shape[0]))[:, None]
        total += int(near.sum())
    return total


def fsum_catalogue(points, labels, count, masses=None, velocities=None, mean_velocity=None):
    """The exact sums behind the catalogue of a non-periodic box, per group: mass = fsum(m),
    moment[d] = fsum of the rounded products m x_d, and with velocities momentum[d] = fsum(m v_d)
    and spread = fsum of the rounded terms m ((dvx dvx + dvy dvy) + dvz dvz) about mean_velocity,
    each with the sum of the terms' magnitudes: {"mass", "moment", "moment_abs", ...}."""
    points = np.asarray(points, dtype=np.float64)
    m_all = np.ones(points.shape[0]) if masses is None else np.asarray(masses, dtype=np.float64)
    out = {"size": [], "mass": [], "mass_abs": [], "moment": [], "moment_abs": [], "momentum": [],
           "momentum_abs": [], "spread": [], "spread_abs": []}
    for g in range(1, count + 1):
        who = np.nonzero(labels == g)[0]
        m = m_all[who]
        out["size"].append(who.size)
        out["mass"].append(math.fsum(m))
        out["mass_abs"].append(math.fsum(np.abs(m)))
        out["moment"].append([math.fsum(m * points[who, d]) for d in range(3)])
        out["moment_abs"].append([math.fsum(np.abs(m * points[who, d])) for d in range(3)])
        if velocities is not None:
            v = np.asarray(velocities, dtype=np.float64)[who]
            out["momentum"].append([math.fsum(m * v[:, d]) for d in range(3)])
            out["momentum_abs"].append([math.fsum(np.abs(m * v[:, d])) for d in range(3)])
            dv = v - np.asarray(mean_velocity, dtype=np.float64)[g - 1]
            terms = m * ((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
            out["spread"].append(math.fsum(terms))
            out["spread_abs"].append(math.fsum(np.abs(terms)))
    return out


U = 2.0 ** -53


def quotient_bound(size, top, top_abs, bottom, bottom_abs):
    """The a-priori bound on |fl(S^ / M^) - S / M| where S^ and M^ are float64 sums of `size` terms
    in any order, S = top and M = bottom > 0 their exact values and top_abs, bottom_abs the sums of
    the terms' magnitudes: each computed sum is within size 2^-53 sum|term| of the exact one
    (Higham, Accuracy and Stability, (4.4): (n - 1) u to first order, here n u with room for the
    higher orders at the test's sizes), and the division adds one rounding.  With eS = size u
    top_abs and eM = size u bottom_abs:  |S^ / M^ - S / M| <= (eS + |S / M| eM) / (M - eM), and the
    rounding of the quotient adds u (|S / M| + that)."""
    e_top = size * U * top_abs
    e_bottom = size * U * bottom_abs
    ratio = abs(top / bottom)
    spread = (e_top + ratio * e_bottom) / (bottom - e_bottom)
    return spread + U * (ratio + spread)
