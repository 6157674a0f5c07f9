"""The reference of the clumps ("Clumps"): plain numpy and a dictionary union-find on
a plotfile's own level arrays, as write_plotfile takes them.

Per loaded level the leaf mask and leaf values of gradient_reference.leaf_arrays.  A leaf cell is
selected iff lower <= v <= upper.  A selected leaf cell of level l with index g is adjacent to,
for each of its six face neighbours n = g +- e: n mapped to levels m = l, l - 1, ..., 0 by floor
division; the first level at which the mapped index is a leaf gives the neighbour cell (inside the
cell's own box that is the next cell, found at m = l); no such level, no neighbour there.  A finer
neighbour is never searched for: it finds the coarse cell from its own side.  The two are united if
the neighbour is selected too.  Clumps are numbered 1..N in ascending order of their smallest
ordinal, a cell's ordinal being cell_begin of its scene box + (k ny + j) nx + i.
"""
import math

import numpy as np

from gradient_reference import leaf_arrays


def ordinal_arrays(levels, scene_boxes):
    """Per level an int64 array over the level's domain: every scene cell's ordinal, -1 elsewhere.
    scene_boxes: (level, lo, hi) in scene order."""
    out = []
    for lev in levels:
        dlo, dhi = lev["domain"]
        out.append(np.full(tuple(dhi[a] - dlo[a] + 1 for a in (2, 1, 0)), -1, dtype=np.int64))
    begin = 0
    for level, lo, hi in scene_boxes:
        dlo = levels[level]["domain"][0]
        shape = tuple(hi[a] - lo[a] + 1 for a in (2, 1, 0))
        count = shape[0] * shape[1] * shape[2]
        cut = tuple(slice(lo[a] - dlo[a], hi[a] - dlo[a] + 1) for a in (2, 1, 0))
        out[level][cut] = begin + np.arange(count, dtype=np.int64).reshape(shape)
        begin += count
    return out, begin


def selected_arrays(arrays, lower, upper):
    with np.errstate(invalid="ignore"):
        return [mask & (values >= lower) & (values <= upper) for _, mask, values in arrays]


def adjacent_pairs(arrays, selected, ref_ratio):
    """Every (cell, neighbour, axis, step) the rule gives with both cells selected; a cell is
    (level, i, j, k), the neighbour lies one step (-1 or +1) along axis past the cell."""
    pairs = []
    for l, (origin, mask, _) in enumerate(arrays):
        k, j, i = np.nonzero(selected[l])
        if not k.size:
            continue
        index = np.stack([i, j, k]).astype(np.int64) + origin[:, None]
        for axis in range(3):
            for step in (-1, 1):
                ghost = index.copy()
                ghost[axis] += step
                found = np.zeros(ghost.shape[1], dtype=bool)
                mapped = ghost
                for m in range(l, -1, -1):
                    if m < l:
                        mapped = mapped // ref_ratio[m]         # floors, also below zero
                    o, leaf, _ = arrays[m]
                    rel = mapped - o[:, None]
                    extent = np.array(leaf.shape[::-1], dtype=np.int64)
                    inside = np.all((rel >= 0) & (rel < extent[:, None]), axis=0)
                    safe = np.where(inside, rel, 0)
                    at = (safe[2], safe[1], safe[0])
                    hit = inside & leaf[at] & ~found
                    take = hit & selected[m][at]
                    for n in np.nonzero(take)[0]:
                        pairs.append(((l, int(index[0, n]), int(index[1, n]), int(index[2, n])),
                                      (m, int(mapped[0, n]), int(mapped[1, n]), int(mapped[2, n])),
                                      axis, step))
                    found |= hit
    return pairs


def clump_levels(levels, ref_ratio, component, lower, upper, scene_boxes, min_level=0,
                 max_level=-1):
    """(labels per level over the level's domain [nz, ny, nx] float64 -- 0.0 where the cell is no
    selected leaf --, N)."""
    arrays, max_level = leaf_arrays(levels, ref_ratio, component, min_level, max_level)
    selected = selected_arrays(arrays, lower, upper)
    ordinals, _ = ordinal_arrays(levels, scene_boxes)
    parent = {}

    def find(x):
        root = x
        while parent.get(root, root) != root:
            root = parent[root]
        while parent.get(x, x) != root:
            parent[x], x = root, parent[x]
        return root

    for a, b, _, _ in adjacent_pairs(arrays, selected, ref_ratio):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[ra] = rb
    # the smallest ordinal of every clump, then the clumps in ascending order of it
    smallest = {}
    cells = []
    for l, (origin, _, _) in enumerate(arrays):
        k, j, i = np.nonzero(selected[l])
        for kk, jj, ii in zip(k.tolist(), j.tolist(), i.tolist()):
            cell = (l, ii + int(origin[0]), jj + int(origin[1]), kk + int(origin[2]))
            ordinal = int(ordinals[l][kk, jj, ii])
            assert ordinal >= 0, "a leaf that is in no scene box"
            root = find(cell)
            cells.append((l, kk, jj, ii, root))
            if root not in smallest or ordinal < smallest[root]:
                smallest[root] = ordinal
    number = {root: n + 1 for n, root in enumerate(sorted(smallest, key=smallest.get))}
    labels = [np.zeros(mask.shape, dtype=np.float64) for _, mask, _ in arrays]
    for l, kk, jj, ii, root in cells:
        labels[l][kk, jj, ii] = float(number[root])
    return labels, len(number)


def clump_table(labels, n, leaf_masks, values=None):
    """The table of per-level label arrays over the leaves (leaf_masks[l] bool): (cells int64 [L,
    n], sums float64 [L, n] by math.fsum or None, abs_sums [L, n], outside, nonfinite) with the
    rules of avr_scene_clump_table."""
    n_levels = len(labels)
    cells = np.zeros((n_levels, n), dtype=np.int64)
    terms = [[[] for _ in range(n)] for _ in range(n_levels)]
    outside = nonfinite = 0
    for l in range(n_levels):
        lab = labels[l][leaf_masks[l]]
        val = None if values is None else values[l][leaf_masks[l]]
        for q, label in enumerate(lab.tolist()):
            if label == 0.0 and not math.copysign(1.0, label) < 0:
                continue
            if not (label >= 1.0 and label <= n and label == math.floor(label)):
                outside += 1
                continue
            if val is not None and not math.isfinite(val[q]):
                nonfinite += 1
                continue
            cells[l, int(label) - 1] += 1
            if val is not None:
                terms[l][int(label) - 1].append(float(val[q]))
    sums = abs_sums = None
    if values is not None:
        sums = np.array([[math.fsum(t) for t in row] for row in terms]).reshape(n_levels, n)
        abs_sums = np.array([[math.fsum(abs(v) for v in t) for t in row]
                             for row in terms]).reshape(n_levels, n)
    return cells, sums, abs_sums, outside, nonfinite
