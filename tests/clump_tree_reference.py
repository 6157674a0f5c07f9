"""The reference of the clump tree ("Clump tree"): plain numpy and Python loops on a
plotfile's own level arrays, as write_plotfile takes them.

Per threshold t[i] the labels of clump_reference.clump_levels over [t[i], upper]; the ladder stops
at the first threshold without a clump.  The parent of clump c of t[i] is read off the label pairs
(label at t[i], label at t[i - 1]) of all cells: every clump must see exactly one parent label,
and it must not be 0.  The extent of a clump comes from a literal loop over its cells: a cell of
level l with index (I, J, K) covers [I R, (I + 1) R - 1] per axis in the index space of the finest
loaded level, R the product of the ratios from l up to it.  Tables are clump_reference.clump_table's.
Nodes are numbered by ascending threshold, then label.
"""
import numpy as np

import clump_reference as cr
from gradient_reference import leaf_arrays


def clump_tree(levels, ref_ratio, component, thresholds, upper, scene_boxes, min_level=0,
               max_level=-1, fields=()):
    """fields: components summed per clump.  Returns a dict: counts (per threshold), labels (per
    threshold with clumps, the per-level label arrays), parent_labels (per threshold an int64
    array; empty for threshold 0 and for thresholds without clumps), parent (node ids, -1 for the
    first threshold's), index_lo, index_hi int64 [n, 3], cells_by_level int64 [L, n], sums and
    abs_sums {component: float64 [L, n]}, nonfinite; L = the finest loaded level + 1."""
    arrays, finest = leaf_arrays(levels, ref_ratio, component, min_level, max_level)
    n_levels = finest + 1
    masks = [mask for _, mask, _ in arrays]
    scale = [int(np.prod(ref_ratio[l:finest], dtype=np.int64)) for l in range(n_levels)]
    counts = [0] * len(thresholds)
    labels, parent_labels = [], [np.zeros(0, dtype=np.int64) for _ in thresholds]
    lows, highs, cells = [], [], []
    sums = {f: [] for f in fields}
    abs_sums = {f: [] for f in fields}
    nonfinite = 0
    for step, threshold in enumerate(thresholds):
        dense, n = cr.clump_levels(levels, ref_ratio, component, threshold, upper, scene_boxes,
                                   min_level, max_level)
        if n == 0:
            break
        counts[step] = n
        lo = np.full((n, 3), np.iinfo(np.int64).max, dtype=np.int64)
        hi = np.full((n, 3), np.iinfo(np.int64).min, dtype=np.int64)
        seen = [set() for _ in range(n)]
        for l in range(n_levels):
            origin = arrays[l][0]
            k, j, i = np.nonzero(dense[l] > 0.0)
            for kk, jj, ii in zip(k.tolist(), j.tolist(), i.tolist()):
                c = int(dense[l][kk, jj, ii]) - 1
                index = (ii + int(origin[0]), jj + int(origin[1]), kk + int(origin[2]))
                for axis in range(3):
                    lo[c, axis] = min(lo[c, axis], index[axis] * scale[l])
                    hi[c, axis] = max(hi[c, axis], (index[axis] + 1) * scale[l] - 1)
                if step > 0:
                    seen[c].add(float(labels[-1][l][kk, jj, ii]))
        if step > 0:
            for c in range(n):
                assert len(seen[c]) == 1 and 0.0 not in seen[c], (threshold, c + 1, seen[c])
            parent_labels[step] = np.array([int(next(iter(s))) for s in seen], dtype=np.int64)
        lows.append(lo)
        highs.append(hi)
        cells.append(cr.clump_table(dense, n, masks)[0][:n_levels])
        for f in fields:
            values = leaf_arrays(levels, ref_ratio, f, min_level, max_level)[0]
            _, summed, absolute, _, bad = cr.clump_table(dense, n, masks, [v for _, _, v in values])
            sums[f].append(summed[:n_levels])
            abs_sums[f].append(absolute[:n_levels])
            nonfinite += bad
        labels.append(dense)
    begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    parent = np.full(int(begin[-1]), -1, dtype=np.int64)
    for step in range(1, len(thresholds)):
        if counts[step]:
            parent[begin[step]:begin[step + 1]] = begin[step - 1] + parent_labels[step] - 1
    no_nodes = np.zeros((0, 3), dtype=np.int64)
    return {"counts": counts, "labels": labels, "parent_labels": parent_labels, "parent": parent,
            "node_begin": begin,
            "index_lo": np.concatenate(lows + [no_nodes]),
            "index_hi": np.concatenate(highs + [no_nodes]),
            "cells_by_level": np.concatenate(cells + [np.zeros((n_levels, 0), dtype=np.int64)],
                                             axis=1),
            "sums": {f: np.concatenate(sums[f] + [np.zeros((n_levels, 0))], axis=1)
                     for f in fields},
            "abs_sums": {f: np.concatenate(abs_sums[f] + [np.zeros((n_levels, 0))], axis=1)
                         for f in fields},
            "nonfinite": nonfinite, "n_levels": n_levels}
