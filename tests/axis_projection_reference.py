"""The float64 numpy reference of the on-axis projection tests (tests/test_axis_projection.py,
tests/test_axis_projection_gpu.py), on a plotfile's own level arrays, not on the convexified
boxes: per loaded level the cells that no grid of the next finer loaded level covers (the masking
of phase_reference), the per-(u, v) column sums along the axis of f (f * w with a weight), w and
the counts, and per pixel floor((p - prob_lo) / dx_l) into each level's plane, summed over the
levels with the level's path length ("On-axis projection")."""
import math

import numpy as np

from phase_reference import clamp, uncovered

AXES = {"x": 0, "y": 1, "z": 2}
MARGIN = 1e-6   # of a finest cell


def image_axes(axis):
    """(U, V) of axis a: x -> (y, z), y -> (z, x), z -> (x, y)."""
    return (axis + 1) % 3, (axis + 2) % 3


def cell_sizes(levels, prob_lo, prob_hi):
    return [tuple((prob_hi[a] - prob_lo[a]) / (lev["domain"][1][a] - lev["domain"][0][a] + 1)
                  for a in range(3)) for lev in levels]


def pixel_lines(center, widths, width, height, axis):
    """(u [W], v [H]) in physical units: center + ((x + 0.5) / W - 0.5) wu, likewise v."""
    au, av = image_axes(axis)
    u = center[au] + ((np.arange(width) + 0.5) / width - 0.5) * widths[0]
    v = center[av] + ((np.arange(height) + 0.5) / height - 0.5) * widths[1]
    return u, v


def clearance(levels, prob_lo, prob_hi, center, widths, width, height, axis):
    """The least distance of a pixel's line from a cell face, in finest cells."""
    au, av = image_axes(axis)
    finest = cell_sizes(levels, prob_lo, prob_hi)[-1]
    u, v = pixel_lines(center, widths, width, height, axis)
    fu = (u - prob_lo[au]) / finest[au]
    fv = (v - prob_lo[av]) / finest[av]
    return min(np.abs(fu - np.rint(fu)).min(), np.abs(fv - np.rint(fv)).min())


def level_terms(levels, level, max_level, f, w):
    """Over the level's whole domain, [nz, ny, nx]: the term of every cell that counts (f, or
    f * w with a weight), its weight, and whether it counts -- uncovered, f (and w) finite."""
    (dlo, dhi) = levels[level]["domain"]
    shape = tuple(dhi[a] - dlo[a] + 1 for a in (2, 1, 0))
    term, weight, counts = np.zeros(shape), np.zeros(shape), np.zeros(shape, bool)
    for (lo, hi), data, mask in zip(levels[level]["boxes"], levels[level]["data"],
                                    uncovered(levels, level, max_level)):
        vf = data[f]
        ok = mask & np.isfinite(vf)
        vw = None
        if w is not None:
            vw = data[w]
            ok &= np.isfinite(vw)
        with np.errstate(invalid="ignore", over="ignore"):
            t = vf * vw if w is not None else vf
        where = tuple(slice(lo[a] - dlo[a], hi[a] - dlo[a] + 1) for a in (2, 1, 0))
        term[where] = np.where(ok, t, 0.0)
        if w is not None:
            weight[where] = np.where(ok, vw, 0.0)
        counts[where] = ok
    return term, weight, counts


def _planes(cube, axis):
    """[nz, ny, nx] -> [n_V, n_U, n_axis]: the cells of a column last."""
    au, av = image_axes(axis)
    return np.transpose(cube, (2 - av, 2 - au, 2 - axis))


def reference(levels, prob_lo, prob_hi, axis, f, w, center, widths, width, height, dl,
              min_level=0, max_level=-1, with_fsum=False):
    """The three images and what the error bound needs.  dl[l]: the path length of level l.
    Returns a dict of [H, W] arrays: integral, weight (zeros without w), length, count (the number
    of cells on the line that count) and, with_fsum, integral_fsum / weight_fsum (math.fsum of
    the terms dl_l * t over every cell of every level on the line) and integral_abs / weight_abs
    (math.fsum of |dl_l * t|)."""
    min_level, max_level = clamp(levels, min_level, max_level)
    au, av = image_axes(axis)
    sizes = cell_sizes(levels, prob_lo, prob_hi)
    u, v = pixel_lines(center, widths, width, height, axis)
    out = {name: np.zeros((height, width)) for name in ("integral", "weight", "length")}
    out["count"] = np.zeros((height, width), np.int64)
    columns = []        # per level: (in_u, in_v, iu, iv, term planes, weight planes, counts)
    for level in range(min_level, max_level + 1):
        term, weight, counts = (_planes(c, axis) for c in level_terms(levels, level, max_level, f, w))
        n_v, n_u, _ = term.shape
        iu = np.floor((u - prob_lo[au]) / sizes[level][au]).astype(np.int64)
        iv = np.floor((v - prob_lo[av]) / sizes[level][av]).astype(np.int64)
        inside = ((iv >= 0) & (iv < n_v))[:, None] & ((iu >= 0) & (iu < n_u))[None, :]
        cu, cv = np.clip(iu, 0, n_u - 1), np.clip(iv, 0, n_v - 1)
        pick = lambda plane: np.where(inside, plane[cv[:, None], cu[None, :]], 0)
        n = pick(counts.sum(axis=2))
        out["integral"] += dl[level] * pick(term.sum(axis=2))
        out["weight"] += dl[level] * pick(weight.sum(axis=2))
        out["length"] += dl[level] * n.astype(np.float64)
        out["count"] += n
        columns.append((level, inside, cu, cv, term, weight, counts))
    if with_fsum:
        for name in ("integral_fsum", "weight_fsum", "integral_abs", "weight_abs"):
            out[name] = np.zeros((height, width))
        for y in range(height):
            for x in range(width):
                ti, tw = [], []
                for level, inside, cu, cv, term, weight, counts in columns:
                    if inside[y, x]:
                        keep = counts[cv[y], cu[x]]
                        ti.extend((dl[level] * term[cv[y], cu[x]][keep]).tolist())
                        tw.extend((dl[level] * weight[cv[y], cu[x]][keep]).tolist())
                assert len(ti) == out["count"][y, x]
                out["integral_fsum"][y, x] = math.fsum(ti)
                out["weight_fsum"][y, x] = math.fsum(tw)
                out["integral_abs"][y, x] = math.fsum(abs(t) for t in ti)
                out["weight_abs"][y, x] = math.fsum(abs(t) for t in tw)
    return out


def brute_force(levels, prob_lo, prob_hi, axis, f, w, center, widths, width, height, dl):
    """The same by Python loops over every cell of every grid of every level: a cell is covered
    when its first fine child lies in a grid of the next level, and it adds to every pixel whose
    line lies inside its (u, v) footprint."""
    au, av = image_axes(axis)
    sizes = cell_sizes(levels, prob_lo, prob_hi)
    u, v = pixel_lines(center, widths, width, height, axis)
    integral, weight, length = (np.zeros((height, width)) for _ in range(3))
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
                        vf = float(data[f][at])
                        vw = float(data[w][at]) if w is not None else 1.0
                        if not (math.isfinite(vf) and math.isfinite(vw)):
                            continue
                        u_lo = prob_lo[au] + cell[au] * sizes[level][au]
                        v_lo = prob_lo[av] + cell[av] * sizes[level][av]
                        for y in np.nonzero((v >= v_lo) & (v < v_lo + sizes[level][av]))[0]:
                            for x in np.nonzero((u >= u_lo) & (u < u_lo + sizes[level][au]))[0]:
                                integral[y, x] += dl[level] * (vf * vw if w is not None else vf)
                                if w is not None:
                                    weight[y, x] += dl[level] * vw
                                length[y, x] += dl[level]
    return integral, weight, length


def bound(n, magnitude):
    """(2 N + 2) 2^-53 sum |term|: the a-priori bound of the products, the dl multiplies and
    recursive summation of N terms in any order."""
    return (2.0 * n + 2.0) * 2.0 ** -53 * magnitude
