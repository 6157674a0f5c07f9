"""The reference of the particle fields ("Particle fields"): plain numpy on a
plotfile's own level arrays, as write_plotfile takes them, applying the definition literally.

A particle's leaf and the presence of a cloud's corners come from streamline_reference.Hierarchy
(locate, leaf, corner), which asks every level's leaf mask and never sees a scene's boxes.  A cell is
named here by its level and its index in that level's index space; the contribution list is built
in the stated order (particle-major, corner-minor) and added per cell in a Python loop over
ascending list index, one IEEE binary64 addition each.
"""
import numpy as np

from streamline_reference import Hierarchy

NGP, CIC = 0, 1
SUM, DENSITY = 0, 1


def hierarchy(levels, ref_ratio, sizes, prob_lo, min_level=0, max_level=-1):
    return Hierarchy(levels, ref_ratio, (0, 0, 0), sizes, prob_lo, min_level, max_level)


def receiving_cell(h, level, index):
    """The same-or-coarser rule for the level-`level` indices index [n, 3]: (present [n], the
    level [n] and the index [n, 3] of the leaf that holds each, junk where none does)."""
    n = index.shape[0]
    present = np.zeros(n, dtype=bool)
    at_level = np.zeros(n, dtype=np.int64)
    at_index = np.zeros((n, 3), dtype=np.int64)
    mapped = index.copy()
    for m in range(level, -1, -1):
        if m < level:
            mapped = mapped // h.ratio[m]               # floors, also below zero
        hit, _ = h.leaf(m, mapped)
        take = hit & ~present
        at_level[take] = m
        at_index[take] = mapped[take]
        present |= hit
    assert np.array_equal(present, h.corner(level, index)[0])
    return present, at_level, at_index


def contributions(h, points, values, method):
    """points [n, 3], values [n] or None -> dict: leaf_level int64 [n] (-1 outside), leaf_index
    [n, 3], level int64 [n, C] and index int64 [n, C, 3] of every entry's cell (level -1: the
    particle is outside), shares float64 [n, C], outside and rerouted (counts)."""
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = points.shape[0]
    v = np.ones(n) if values is None else np.ascontiguousarray(values, dtype=np.float64)
    leaf_level, q, leaf_index = h.locate(points)
    entries = 8 if method == CIC else 1
    level = np.full((n, entries), -1, dtype=np.int64)
    index = np.zeros((n, entries, 3), dtype=np.int64)
    shares = np.zeros((n, entries))
    rerouted = 0
    inside = leaf_level >= 0
    if method == NGP:
        level[inside, 0] = leaf_level[inside]
        index[inside, 0] = leaf_index[inside]
        shares[inside, 0] = v[inside]
    else:
        for l in range(h.max_level + 1):
            pick = np.nonzero(leaf_level == l)[0]
            if not pick.size:
                continue
            u = q[pick] - 0.5
            base = np.floor(u).astype(np.int64)
            w = u - base.astype(np.float64)
            for c in range(8):
                step = np.array([c & 1, (c >> 1) & 1, c >> 2], dtype=np.int64)
                weight = [w[:, d] if step[d] else 1.0 - w[:, d] for d in range(3)]
                with np.errstate(all="ignore"):
                    shares[pick, c] = ((weight[0] * weight[1]) * weight[2]) * v[pick]
                present, at_level, at_index = receiving_cell(h, l, base + step[None, :])
                level[pick, c] = np.where(present, at_level, l)
                index[pick, c] = np.where(present[:, None], at_index, leaf_index[pick])
                rerouted += int((~present).sum())
    return {"leaf_level": leaf_level, "leaf_index": leaf_index, "level": level, "index": index,
            "shares": shares, "outside": int((~inside).sum()), "rerouted": rerouted}


def deposit(h, found, quantity):
    """The contributions added per cell in ascending list index: per level a float64 array over
    the level's domain [nz, ny, nx] (what Hierarchy's masks cover), +0.0 where nothing lands."""
    dense = [np.zeros(mask.shape) for mask in h.mask]
    level = found["level"].reshape(-1)
    index = found["index"].reshape(-1, 3)
    shares = found["shares"].reshape(-1)
    with np.errstate(all="ignore"):
        for e in range(level.size):
            l = int(level[e])
            if l < 0:
                continue
            i, j, k = (int(x) for x in index[e] - h.origin[l])
            dense[l][k, j, i] = dense[l][k, j, i] + shares[e]
        if quantity == DENSITY:
            for l in range(len(dense)):
                volume = (h.dx[l][0] * h.dx[l][1]) * h.dx[l][2]
                dense[l] = dense[l] / volume
    return dense


def deposit_levels(levels, ref_ratio, sizes, prob_lo, points, values, method, quantity,
                   min_level=0, max_level=-1):
    """(dense per level, outside, rerouted) of one call."""
    h = hierarchy(levels, ref_ratio, sizes, prob_lo, min_level, max_level)
    found = contributions(h, points, values, method)
    return deposit(h, found, quantity), found["outside"], found["rerouted"]
