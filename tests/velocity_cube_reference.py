"""The float64 numpy reference of the velocity cube tests (tests/test_velocity_cube.py,
tests/test_velocity_cube_gpu.py), on a plotfile's own level arrays and built on
axis_projection_reference: the same uncovered cells, pixel lines and per-level columns.  Per cell
that counts the terms of DESIGN.md 7, "Velocity cubes": sharp cells by searchsorted against the
edges (the last channel closed at the top), broadened cells by math.erf (through numpy.vectorize)
of the three-operation argument with the clamp at +-6."""
import math

import numpy as np

import axis_projection_reference as ref
from axis_projection_reference import _planes, clearance, pixel_lines  # noqa: F401 (re-exported)
from phase_reference import bin_of, clamp, uncovered

ERF = np.vectorize(math.erf, otypes=[np.float64])
RSQRT2 = 0.70710678118654752440


def profile(edges, g, s):
    """q [n, nc + 1] of cells with s > 0: the clamped erf of ((edges - g) / s) * RSQRT2."""
    with np.errstate(over="ignore", divide="ignore"):
        a = ((edges[None, :] - g[:, None]) / s[:, None]) * RSQRT2
    inner = (a > -6.0) & (a < 6.0)
    q = np.where(a <= -6.0, -1.0, 1.0)
    q[inner] = ERF(a[inner])
    return q


def cell_terms(e, g, s, edges):
    """[n, nc + 2]: what each of n cells that count adds to the nc channels, to under and to over.
    s: None (every cell sharp) or the widths, >= 0."""
    nc = edges.size - 1
    terms = np.zeros((e.size, nc + 2))
    sharp = np.ones(e.size, bool) if s is None else s == 0.0
    rows = np.nonzero(sharp)[0]
    under, over = g[rows] < edges[0], g[rows] > edges[-1]
    inside = rows[~under & ~over]
    terms[inside, bin_of(edges, g[inside])] = e[inside]
    terms[rows[under], nc] = e[rows[under]]
    terms[rows[over], nc + 1] = e[rows[over]]
    rows = np.nonzero(~sharp)[0]
    if rows.size:
        q = profile(edges, g[rows], s[rows])
        terms[rows, :nc] = e[rows, None] * (0.5 * (q[:, 1:] - q[:, :-1]))
        terms[rows, nc] = e[rows] * (0.5 * (q[:, 0] + 1.0))
        terms[rows, nc + 1] = e[rows] * (0.5 * (1.0 - q[:, -1]))
    return terms


def level_cells(levels, level, max_level, e, g, s):
    """Over the level's whole domain, [nz, ny, nx]: e, g, s (zeros without s) and whether the cell
    counts -- uncovered, e and g finite and, with s, s finite and >= 0."""
    (dlo, dhi) = levels[level]["domain"]
    shape = tuple(dhi[a] - dlo[a] + 1 for a in (2, 1, 0))
    ve, vg, vs, counts = np.zeros(shape), np.zeros(shape), np.zeros(shape), np.zeros(shape, bool)
    for (lo, hi), data, mask in zip(levels[level]["boxes"], levels[level]["data"],
                                    uncovered(levels, level, max_level)):
        ok = mask & np.isfinite(data[e]) & np.isfinite(data[g])
        if s is not None:
            with np.errstate(invalid="ignore"):
                ok &= np.isfinite(data[s]) & (data[s] >= 0.0)
        where = tuple(slice(lo[a] - dlo[a], hi[a] - dlo[a] + 1) for a in (2, 1, 0))
        ve[where] = np.where(ok, data[e], 0.0)
        vg[where] = np.where(ok, data[g], 0.0)
        if s is not None:
            vs[where] = np.where(ok, data[s], 0.0)
        counts[where] = ok
    return ve, vg, vs, counts


def reference(levels, prob_lo, prob_hi, axis, e, g, s, center, widths, width, height, dl, edges,
              min_level=0, max_level=-1, with_fsum=False):
    """e, g, s: component indices (s None: no width field).  Returns a dict: cube [nc, H, W],
    under, over, length [H, W] (numpy sums per level, the levels added in ascending order), count
    [H, W] (the cells on the line that count) and, with_fsum, fsum and abs [nc + 2, H, W]
    (math.fsum of the terms dl_l * t, and of their absolute values, per channel, then under, then
    over), A [H, W] = fsum(dl_l |e|) and E [H, W] = fsum(dl_l e) over the cells that count."""
    edges = np.asarray(edges, dtype=np.float64)
    nc = edges.size - 1
    min_level, max_level = clamp(levels, min_level, max_level)
    au, av = ref.image_axes(axis)
    sizes = ref.cell_sizes(levels, prob_lo, prob_hi)
    u, v = pixel_lines(center, widths, width, height, axis)
    total = np.zeros((nc + 2, height, width))
    out = {"length": np.zeros((height, width)), "count": np.zeros((height, width), np.int64)}
    if with_fsum:
        out["fsum"], out["abs"] = np.zeros((nc + 2, height, width)), np.zeros((nc + 2, height, width))
        out["A"], out["E"] = np.zeros((height, width)), np.zeros((height, width))
    per_pixel = [[[] for _ in range(width)] for _ in range(height)]   # (dl * terms, dl * e)
    for level in range(min_level, max_level + 1):
        ve, vg, vs, counts = (_planes(c, axis) for c in level_cells(levels, level, max_level, e, g, s))
        n_v, n_u, _ = ve.shape
        iu = np.floor((u - prob_lo[au]) / sizes[level][au]).astype(np.int64)
        iv = np.floor((v - prob_lo[av]) / sizes[level][av]).astype(np.int64)
        columns = {}
        for y in range(height):
            if not 0 <= iv[y] < n_v:
                continue
            for x in range(width):
                if not 0 <= iu[x] < n_u:
                    continue
                key = (iv[y], iu[x])
                if key not in columns:
                    keep = counts[key]
                    terms = cell_terms(ve[key][keep], vg[key][keep],
                                       None if s is None else vs[key][keep], edges)
                    columns[key] = (terms, terms.sum(axis=0), ve[key][keep])
                terms, sums, emission = columns[key]
                total[:, y, x] += dl[level] * sums
                out["length"][y, x] += dl[level] * float(terms.shape[0])
                out["count"][y, x] += terms.shape[0]
                if with_fsum:
                    per_pixel[y][x].append((dl[level] * terms, dl[level] * emission))
    if with_fsum:
        for y in range(height):
            for x in range(width):
                if per_pixel[y][x]:
                    terms = np.vstack([t for t, _ in per_pixel[y][x]])
                    for c in np.nonzero(terms.any(axis=0))[0]:
                        column = terms[:, c].tolist()
                        out["fsum"][c, y, x] = math.fsum(column)
                        out["abs"][c, y, x] = math.fsum(abs(t) for t in column)
                    emission = np.concatenate([m for _, m in per_pixel[y][x]]).tolist()
                    out["E"][y, x] = math.fsum(emission)
                    out["A"][y, x] = math.fsum(abs(t) for t in emission)
    out["cube"], out["under"], out["over"] = total[:nc], total[nc], total[nc + 1]
    return out


def brute_force(levels, prob_lo, prob_hi, axis, e, g, s, center, widths, width, height, dl, edges):
    """The same by Python loops over every cell of every grid of every level, in scalar arithmetic:
    a cell is covered when its first fine child lies in a grid of the next level, it adds to every
    pixel whose line lies inside its (u, v) footprint, and its channel is found by walking the
    edges."""
    edges = [float(x) for x in edges]
    nc = len(edges) - 1
    au, av = ref.image_axes(axis)
    sizes = ref.cell_sizes(levels, prob_lo, prob_hi)
    u, v = pixel_lines(center, widths, width, height, axis)
    total = np.zeros((nc + 2, height, width))
    length = np.zeros((height, width))
    for level in range(len(levels)):
        fine = levels[level + 1]["boxes"] if level + 1 < len(levels) else []
        for (lo, hi), data in zip(levels[level]["boxes"], levels[level]["data"]):
            for k in range(lo[2], hi[2] + 1):
                for j in range(lo[1], hi[1] + 1):
                    for i in range(lo[0], hi[0] + 1):
                        cell = (i, j, k)
                        if any(all(flo[a] <= 2 * cell[a] <= fhi[a] for a in range(3))
                               for flo, fhi in fine):
                            continue
                        at = (k - lo[2], j - lo[1], i - lo[0])
                        ve, vg = float(data[e][at]), float(data[g][at])
                        vs = float(data[s][at]) if s is not None else 0.0
                        if not (math.isfinite(ve) and math.isfinite(vg) and math.isfinite(vs)
                                and vs >= 0.0):
                            continue
                        terms = [0.0] * (nc + 2)
                        if vs == 0.0:
                            if vg < edges[0]:
                                terms[nc] = ve
                            elif vg > edges[nc]:
                                terms[nc + 1] = ve
                            else:
                                c = 0
                                while c + 1 < nc and edges[c + 1] <= vg:
                                    c += 1
                                terms[c] = ve
                        else:
                            q = []
                            for edge in edges:
                                t = (edge - vg) / vs
                                a = t * RSQRT2
                                q.append(-1.0 if a <= -6.0 else 1.0 if a >= 6.0 else math.erf(a))
                            for c in range(nc):
                                terms[c] = ve * (0.5 * (q[c + 1] - q[c]))
                            terms[nc] = ve * (0.5 * (q[0] + 1.0))
                            terms[nc + 1] = ve * (0.5 * (1.0 - q[nc]))
                        u_lo = prob_lo[au] + cell[au] * sizes[level][au]
                        v_lo = prob_lo[av] + cell[av] * sizes[level][av]
                        for y in np.nonzero((v >= v_lo) & (v < v_lo + sizes[level][av]))[0]:
                            for x in np.nonzero((u >= u_lo) & (u < u_lo + sizes[level][au]))[0]:
                                total[:, y, x] += dl[level] * np.array(terms)
                                length[y, x] += dl[level]
    return total[:nc], total[nc], total[nc + 1], length


def bound(n, magnitude):
    """(2 N + 2) 2^-53 sum |term|: the projection's a-priori bound."""
    return ref.bound(n, magnitude)


def erf_bound(a_total):
    """22 * 2^-53 * A: 16 ulp of |q| <= 1 for the device's erf, under 1.5 for the three argument
    roundings (max |a erf'(a)| = 0.484), 0.5 for the clamp, 1 for the subtraction and the halving,
    1 for math.erf here; rounded up."""
    return 22.0 * 2.0 ** -53 * a_total
