"""The reference of the isosurfaces ("Isosurface"): plain numpy on a plotfile's own
level arrays, as write_plotfile takes them, applying the definition literally.

Per loaded level the leaf mask and leaf values of gradient_reference.leaf_arrays.  The value at a
level-l index G is that of the first level m = l, l - 1, ..., 0 at which G, mapped down by floor
division, is a leaf; none: absent.  A corner sits at prob_lo + (f64(G) + 0.5) * dx[l] whichever
level gave its value.  Scene box b of level l enumerates the cube bases [lo - 1, hi] along every
axis, k slowest; a cube is kept iff all eight corners are present and the lowest-numbered corner
that is a level-l leaf lies in b.  A kept cube with a corner that is not finite is skipped.  The
tables below are literals: the six tetrahedra as paths of corner numbers (c = di + 2 dj + 4 dk),
per case (bit n: path vertex n is inside, v >= value) the cut edges in the order of the rule, and
whether the last two vertices of the case's triangles are swapped in a tetrahedron whose path
takes the axes in an even permutation of (x, y, z); in an odd one the opposite holds.
"""
import numpy as np

from gradient_reference import leaf_arrays

TETS = ((0, 1, 3, 7), (0, 1, 5, 7), (0, 2, 3, 7), (0, 2, 6, 7), (0, 4, 5, 7), (0, 4, 6, 7))
TET_ODD = (0, 1, 1, 0, 0, 1)
# one inside vertex a, the others p < q < r: E(a,p) E(a,q) E(a,r); three inside: the same from the
# one outside vertex; two inside a < b, outside p < q: E(a,p) E(a,q) E(b,q) E(b,p)
EDGES = (
    (),
    ((0, 1), (0, 2), (0, 3)),
    ((1, 0), (1, 2), (1, 3)),
    ((0, 2), (0, 3), (1, 3), (1, 2)),
    ((2, 0), (2, 1), (2, 3)),
    ((0, 1), (0, 3), (2, 3), (2, 1)),
    ((1, 0), (1, 3), (2, 3), (2, 0)),
    ((3, 0), (3, 1), (3, 2)),
    ((3, 0), (3, 1), (3, 2)),
    ((0, 1), (0, 2), (3, 2), (3, 1)),
    ((1, 0), (1, 2), (3, 2), (3, 0)),
    ((2, 0), (2, 1), (2, 3)),
    ((2, 0), (2, 1), (3, 1), (3, 0)),
    ((1, 0), (1, 2), (1, 3)),
    ((0, 1), (0, 2), (0, 3)),
    (),
)
SWAP_EVEN = (0, 0, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 1, 0)


def case_triangles(tet, mask):
    """The triangles of case `mask` in tetrahedron `tet`: triples of cut edges (x, y), path
    vertices of the tetrahedron, oriented."""
    edges = EDGES[mask]
    if not edges:
        return []
    triangles = [(edges[0], edges[1], edges[2])]
    if len(edges) == 4:
        triangles.append((edges[0], edges[2], edges[3]))
    if SWAP_EVEN[mask] ^ TET_ODD[tet]:
        triangles = [(a, c, b) for a, b, c in triangles]
    return triangles


def lookup(arrays, others, ref_ratio, level, index):
    """The corner rule for the level-`level` indices index [3, n]: (present [n], the level that
    gave the value [n] (-1 if absent), value [n], value of `others` [n] or None).  others: the
    leaf arrays of a second field over the same leaves, or None."""
    n = index.shape[1]
    found = np.full(n, -1, dtype=np.int64)
    value = np.zeros(n, dtype=np.float64)
    second = np.zeros(n, dtype=np.float64) if others is not None else None
    mapped = index.copy()
    for m in range(level, -1, -1):
        if m < level:
            mapped = mapped // ref_ratio[m]             # floors, also below zero
        origin, mask, values = arrays[m]
        rel = mapped - origin[:, None]
        extent = np.array(mask.shape[::-1], dtype=np.int64)
        inside = np.all((rel >= 0) & (rel < extent[:, None]), axis=0)
        safe = np.where(inside, rel, 0)
        at = (safe[2], safe[1], safe[0])
        take = inside & mask[at] & (found < 0)
        value[take] = values[at][take]
        if others is not None:
            second[take] = others[m][2][at][take]
        found[take] = m
    return found >= 0, found, value, second


def box_cubes(arrays, others, ref_ratio, level, lo, hi):
    """The cube bases of scene box (level, lo, hi), k slowest: (bases [3, n], kept [n], corner
    values [8, n], corner sample values [8, n] or None, corner indices [8, 3, n])."""
    k, j, i = np.meshgrid(np.arange(lo[2] - 1, hi[2] + 1), np.arange(lo[1] - 1, hi[1] + 1),
                          np.arange(lo[0] - 1, hi[0] + 1), indexing="ij")
    bases = np.stack([i.ravel(), j.ravel(), k.ravel()]).astype(np.int64)
    n = bases.shape[1]
    present = np.ones(n, dtype=bool)
    decided = np.zeros(n, dtype=bool)
    owned = np.zeros(n, dtype=bool)
    values = np.zeros((8, n))
    samples = np.zeros((8, n)) if others is not None else None
    corners = np.zeros((8, 3, n), dtype=np.int64)
    low = np.array(lo, dtype=np.int64)[:, None]
    high = np.array(hi, dtype=np.int64)[:, None]
    for c in range(8):
        index = bases + np.array([[c & 1], [(c >> 1) & 1], [c >> 2]], dtype=np.int64)
        corners[c] = index
        there, found, values[c], second = lookup(arrays, others, ref_ratio, level, index)
        if others is not None:
            samples[c] = second
        present &= there
        own = np.all((index >= low) & (index <= high), axis=0)
        assert (found[own] == level).all(), "a scene box holds a cell that is no leaf"
        same_level = found == level
        owned |= same_level & ~decided & own
        decided |= same_level
    return bases, present & owned, values, samples, corners


def isosurface(levels, ref_ratio, component, value, scene_boxes, sizes, prob_lo, min_level=0,
               max_level=-1, sample_component=None):
    """scene_boxes: (level, lo, hi) in scene order; sizes[l] = (dx, dy, dz).  Returns a dict:
    vertices [T, 3, 3], level uint8 [T], samples [T, 3] or None, skipped, and cubes, the list of
    (scene box, level, (i, j, k)) of every kept cube in output order."""
    arrays, max_level = leaf_arrays(levels, ref_ratio, component, min_level, max_level)
    others = None
    if sample_component is not None:
        others = leaf_arrays(levels, ref_ratio, sample_component, min_level, max_level)[0]
    value = np.float64(value)
    origin = np.array(prob_lo, dtype=np.float64)
    out_v, out_l, out_s, cubes = [], [], [], []
    skipped = 0
    for b, (level, lo, hi) in enumerate(scene_boxes):
        bases, kept, values, samples, corners = box_cubes(arrays, others, ref_ratio, level, lo, hi)
        for q in np.nonzero(kept)[0]:
            cubes.append((b, level, tuple(int(v) for v in bases[:, q])))
        finite = np.isfinite(values).all(axis=0)
        skipped += int((kept & ~finite).sum())
        live = np.nonzero(kept & finite)[0]
        if not live.size:
            continue
        values = values[:, live]
        corners = corners[:, :, live]
        if samples is not None:
            samples = samples[:, live]
        dx = np.array(sizes[level], dtype=np.float64)
        # a corner's position, nothing fused
        position = origin[None, :, None] + (corners.astype(np.float64) + 0.5) * dx[None, :, None]
        inside = values >= value
        keys, soup, sampled = [], [], []
        rank = np.arange(live.size, dtype=np.int64)
        for t, tet in enumerate(TETS):
            mask = sum(inside[c].astype(np.int64) << n for n, c in enumerate(tet))
            for case in range(1, 15):
                pick = np.nonzero(mask == case)[0]
                if not pick.size:
                    continue
                for number, triangle in enumerate(case_triangles(t, case)):
                    points = np.zeros((pick.size, 3, 3))
                    at_points = np.zeros((pick.size, 3))
                    for corner, (x, y) in enumerate(triangle):
                        cx, cy = tet[x], tet[y]
                        vx, vy = values[cx, pick], values[cy, pick]
                        x_low = vx < value
                        assert (x_low != (vy < value)).all()
                        v_lo, v_hi = np.where(x_low, vx, vy), np.where(x_low, vy, vx)
                        with np.errstate(all="ignore"):
                            s = (value - v_lo) / (v_hi - v_lo)
                            p_lo = np.where(x_low, position[cx][:, pick], position[cy][:, pick])
                            p_hi = np.where(x_low, position[cy][:, pick], position[cx][:, pick])
                            points[:, corner, :] = (p_lo + s * (p_hi - p_lo)).T
                            if samples is not None:
                                sx, sy = samples[cx, pick], samples[cy, pick]
                                s_lo, s_hi = np.where(x_low, sx, sy), np.where(x_low, sy, sx)
                                at_points[:, corner] = s_lo + s * (s_hi - s_lo)
                    keys.append(rank[pick] * 12 + t * 2 + number)
                    soup.append(points)
                    sampled.append(at_points)
        if keys:
            order = np.argsort(np.concatenate(keys), kind="stable")
            out_v.append(np.concatenate(soup)[order])
            out_s.append(np.concatenate(sampled)[order])
            out_l.append(np.full(order.size, level, dtype=np.uint8))
    vertices = np.concatenate(out_v) if out_v else np.zeros((0, 3, 3))
    return {"vertices": vertices,
            "level": np.concatenate(out_l) if out_l else np.zeros(0, dtype=np.uint8),
            "samples": None if sample_component is None else
            (np.concatenate(out_s) if out_s else np.zeros((0, 3))),
            "skipped": skipped, "cubes": cubes}
