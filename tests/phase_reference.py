"""Fixtures and the float64 numpy reference of the joint-histogram tests (tests/test_phase.py,
tests/test_phase_gpu.py).  The reference works on a plotfile's own level arrays, not on the
convexified boxes: per loaded level the cells that no grid of the next finer loaded level covers
(the fine boxes coarsened by the ratio), then the per-cell rule of DESIGN.md 7, "Phase plot and
profile", with numpy.searchsorted."""
import math

import numpy as np

PROB_LO = (0.3, -1.1, 2.0)
PROB_HI = (1.7, 0.1, 3.05)
VARIABLES = ["density", "temperature", "energy", "count"]
RATIO = 2

# explicit, non-uniform edges; the fixtures plant cells exactly on every one of them
X_EDGES = np.array([-250.0, -100.5, -30.0, -1.0, 0.0, 0.125, 7.0, 55.5, 100.0, 260.0])
Y_EDGES = np.array([1e-3, 0.02, 0.5, 1.0, 3.75, 40.0, 1e3])


def linear_edges(lo, hi, n):
    """The issue's formula, restated: e[i] = lo + (hi - lo) * (i / n), e[n] = hi."""
    e = np.float64(lo) + (np.float64(hi) - np.float64(lo)) * (np.arange(n + 1) / np.float64(n))
    e[n] = hi
    return e


def log_edges(lo, hi, n):
    a, b = np.log10(np.float64(lo)), np.log10(np.float64(hi))
    e = np.float64(10.0) ** (a + (b - a) * (np.arange(n + 1) / np.float64(n)))
    e[0], e[n] = lo, hi
    return e


# values planted into the x (component 0) and y (component 1) fields: every edge of the explicit
# arrays and of the generated ones the tests use
PLANTED_X = np.concatenate([X_EDGES, linear_edges(-300.0, 300.0, 7),
                            linear_edges(-300.0, 300.0, 128)[::9],
                            linear_edges(-300.0, 300.0, 1024)[::93], [-300.0, 300.0]])
PLANTED_Y = np.concatenate([Y_EDGES, log_edges(1e-3, 1e3, 5), log_edges(1e-3, 1e3, 128)[::9],
                            log_edges(1e-3, 1e3, 1024)[::93], [1e-3, 1e3]])


def _cells(rng, box, cursor):
    """[4, nz, ny, nx]: density ~ 100 N(0, 1), temperature lognormal (positive, five decades),
    energy ~ 1000 N(0, 1), count = integers in [-2^20, 2^20].  About 8 % of density and temperature
    lie exactly on bin edges (the planted values in turn; cursor counts them across grids); about
    2 % of every field, independently, are NaN / +Inf / -Inf."""
    lo, hi = box
    shape = (hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1)
    n = shape[0] * shape[1] * shape[2]
    data = np.empty((4,) + shape, np.float64)
    data[0] = rng.standard_normal(shape) * 100.0
    data[1] = np.exp(rng.standard_normal(shape) * 2.5)
    data[2] = rng.standard_normal(shape) * 1000.0
    data[3] = rng.integers(-2 ** 20, 2 ** 20 + 1, size=shape).astype(np.float64)
    for comp, planted in ((0, PLANTED_X), (1, PLANTED_Y)):
        at = rng.choice(n, max(n // 12, 4), replace=False)
        data[comp].reshape(-1)[at] = planted[(cursor[comp] + np.arange(at.size)) % planted.size]
        cursor[comp] += at.size
    for comp in range(4):
        odd = rng.choice(n, max(n // 50, 3), replace=False)
        data[comp].reshape(-1)[odd] = np.array([np.nan, np.inf, -np.inf])[np.arange(odd.size) % 3]
    return data


def three_levels(seed=2025):
    """12 x 10 x 8 coarse cells in two grids (7 and 5 cells wide: odd row strides), two level-1
    grids and two level-2 grids inside them, all non-cubic."""
    rng, cursor = np.random.default_rng(seed), [0, 0]
    boxes = [
        [((0, 0, 0), (6, 9, 7)), ((7, 0, 0), (11, 9, 7))],
        [((4, 4, 2), (13, 11, 9)), ((14, 6, 4), (19, 15, 11))],
        [((12, 10, 6), (23, 19, 13)), ((30, 14, 10), (37, 25, 19))],
    ]
    domains = [((0, 0, 0), (11, 9, 7)), ((0, 0, 0), (23, 19, 15)), ((0, 0, 0), (47, 39, 31))]
    return [{"domain": d, "boxes": b, "data": [_cells(rng, box, cursor) for box in b]}
            for d, b in zip(domains, boxes)]


def many_boxes(seed=78):
    """16^3 coarse cells with 64 refined islands: far more than 169 convexified boxes."""
    rng, cursor = np.random.default_rng(seed), [0, 0]
    coarse = [((0, 0, 0), (15, 15, 15))]
    fine = [((8 * a + 2, 8 * b + 2, 8 * c + 2), (8 * a + 5, 8 * b + 5, 8 * c + 5))
            for c in range(4) for b in range(4) for a in range(4)]
    return [{"domain": ((0, 0, 0), (15, 15, 15)), "boxes": coarse,
             "data": [_cells(rng, box, cursor) for box in coarse]},
            {"domain": ((0, 0, 0), (31, 31, 31)), "boxes": fine,
             "data": [_cells(rng, box, cursor) for box in fine]}]


def tiny_levels():
    """4 x 3 x 2 coarse cells, one 4 x 2 x 2 fine grid over two of them columns."""
    rng, cursor = np.random.default_rng(5), [0, 0]
    boxes = [[((0, 0, 0), (3, 2, 1))], [((2, 2, 0), (5, 3, 1))]]
    domains = [((0, 0, 0), (3, 2, 1)), ((0, 0, 0), (7, 5, 3))]
    return [{"domain": d, "boxes": b, "data": [_cells(rng, box, cursor) for box in b]}
            for d, b in zip(domains, boxes)]


def write(path, levels):
    from amrvolumerenderer_amd import plotfile
    plotfile.write_plotfile(str(path), VARIABLES, levels, PROB_LO, PROB_HI,
                            [RATIO] * (len(levels) - 1))
    return str(path)


def cell_sizes(levels):
    return [tuple((PROB_HI[a] - PROB_LO[a]) / (lev["domain"][1][a] - lev["domain"][0][a] + 1)
                  for a in range(3)) for lev in levels]


def volumes(levels):
    """vol[l] = dx * dy * dz, multiplied in this order."""
    return [c[0] * c[1] * c[2] for c in cell_sizes(levels)]


def clamp(levels, min_level, max_level):
    finest = len(levels) - 1
    if max_level < 0 or max_level > finest:
        max_level = finest
    return min(max(min_level, 0), finest), max_level


def uncovered(levels, level, max_level):
    """Per grid of `level` the [nz, ny, nx] mask of cells no grid of level + 1 covers (every cell
    if level + 1 is not loaded)."""
    masks = []
    for lo, hi in levels[level]["boxes"]:
        mask = np.ones((hi[2] - lo[2] + 1, hi[1] - lo[1] + 1, hi[0] - lo[0] + 1), bool)
        if level + 1 <= max_level:
            for flo, fhi in levels[level + 1]["boxes"]:
                clo = [max(flo[a] // RATIO, lo[a]) for a in range(3)]
                chi = [min(fhi[a] // RATIO, hi[a]) for a in range(3)]
                if all(clo[a] <= chi[a] for a in range(3)):
                    mask[clo[2] - lo[2]:chi[2] - lo[2] + 1, clo[1] - lo[1]:chi[1] - lo[1] + 1,
                         clo[0] - lo[0]:chi[0] - lo[0] + 1] = False
        masks.append(mask)
    return masks


def bin_of(edges, v):
    """numpy.searchsorted(e, v, "right") - 1, the last bin closed at the top."""
    i = np.searchsorted(edges, v, "right") - 1
    i[v == edges[-1]] = len(edges) - 2
    return i


def reference(levels, x, y, s, x_edges, y_edges, min_level=0, max_level=-1):
    """The joint histogram of components x, y (None: one y bin) and s (None: no sums) of the level
    arrays.  Returns a dict: cells int64 [L, ny, nx], outside, nonfinite, uncovered (the number of
    uncovered cells of the loaded levels) and, with s, per level a dict bin -> the values summed
    there (`terms`, flat bin = by * nx + bx)."""
    min_level, max_level = clamp(levels, min_level, max_level)
    nx = len(x_edges) - 1
    ny = 1 if y is None else len(y_edges) - 1
    cells = np.zeros((max_level + 1, ny * nx), np.int64)
    terms = [dict() for _ in range(max_level + 1)]
    outside = nonfinite = total = 0
    for level in range(min_level, max_level + 1):
        for data, mask in zip(levels[level]["data"], uncovered(levels, level, max_level)):
            vx = data[x][mask]
            vy = data[y][mask] if y is not None else None
            vs = data[s][mask] if s is not None else None
            total += vx.size
            finite = np.isfinite(vx)
            if vy is not None:
                finite &= np.isfinite(vy)
            if vs is not None:
                finite &= np.isfinite(vs)
            nonfinite += int((~finite).sum())
            inside = finite & (vx >= x_edges[0]) & (vx <= x_edges[-1])
            if vy is not None:
                inside &= (vy >= y_edges[0]) & (vy <= y_edges[-1])
            outside += int((finite & ~inside).sum())
            flat = bin_of(x_edges, vx[inside])
            if vy is not None:
                flat = flat + bin_of(y_edges, vy[inside]) * nx
            np.add.at(cells[level], flat, 1)
            if vs is not None:
                for b, v in zip(flat.tolist(), vs[inside].tolist()):
                    terms[level].setdefault(b, []).append(v)
    return {"cells": cells.reshape(max_level + 1, ny, nx), "outside": outside,
            "nonfinite": nonfinite, "uncovered": total, "terms": terms if s is not None else None}


def brute_force(levels, x, y, s, x_edges, y_edges):
    """The same by a Python loop over every cell of every grid of every level: a cell is covered
    when its first fine child (index * ratio) lies in a grid of the next level (the fine grids
    start and end on coarse cell faces), and its bin is found by walking the edges."""
    n_levels = len(levels)
    nx = len(x_edges) - 1
    ny = 1 if y is None else len(y_edges) - 1
    cells = np.zeros((n_levels, ny, nx), np.int64)
    sums = [dict() for _ in range(n_levels)]
    outside = nonfinite = total = 0

    def locate(edges, v):
        if v < edges[0] or v > edges[-1]:
            return None
        for i in range(len(edges) - 1):
            if edges[i] <= v < edges[i + 1]:
                return i
        return len(edges) - 2       # v == e[n]

    for level in range(n_levels):
        fine = levels[level + 1]["boxes"] if level + 1 < n_levels else []
        for (lo, hi), data in zip(levels[level]["boxes"], levels[level]["data"]):
            for k in range(lo[2], hi[2] + 1):
                for j in range(lo[1], hi[1] + 1):
                    for i in range(lo[0], hi[0] + 1):
                        child = (i * RATIO, j * RATIO, k * RATIO)
                        if any(all(flo[a] <= child[a] <= fhi[a] for a in range(3))
                               for flo, fhi in fine):
                            continue
                        total += 1
                        at = (k - lo[2], j - lo[1], i - lo[0])
                        vx = float(data[x][at])
                        vy = float(data[y][at]) if y is not None else 0.0
                        vs = float(data[s][at]) if s is not None else 0.0
                        if not (math.isfinite(vx) and math.isfinite(vy) and math.isfinite(vs)):
                            nonfinite += 1
                            continue
                        bx = locate(x_edges, vx)
                        by = locate(y_edges, vy) if y is not None else 0
                        if bx is None or by is None:
                            outside += 1
                            continue
                        cells[level, by, bx] += 1
                        sums[level].setdefault(by * nx + bx, []).append(vs)
    return {"cells": cells, "outside": outside, "nonfinite": nonfinite, "uncovered": total,
            "terms": sums if s is not None else None}


def check_sums(got, ref, exact):
    """got: float64 [L, ny, nx] from the device; ref: reference()'s dict.  exact: every bin's sum
    must equal math.fsum of its terms bit for bit (a field of small integers: every partial sum is
    exact in any order).  Otherwise |got - fsum| <= (n - 1) * 2^-53 * sum |v| + half an ulp of the
    reference: the textbook a-priori bound for recursive summation of n terms in any order (Higham,
    Accuracy and Stability of Numerical Algorithms, 4.2) plus the one rounding of the correctly
    rounded reference sum -- not a measured tolerance.  Every bin is checked; a bin without cells
    must hold +0.0.  Returns the largest error / bound ratio seen (0 if exact)."""
    n_levels, ny, nx = ref["cells"].shape
    assert got.shape == (n_levels, ny, nx) and got.dtype == np.float64
    flat = got.reshape(n_levels, ny * nx)
    seen = np.zeros(flat.shape, bool)
    worst = 0.0
    for level in range(n_levels):
        for b, values in ref["terms"][level].items():
            seen[level, b] = True
            want = math.fsum(values)
            assert len(values) == ref["cells"].reshape(n_levels, -1)[level, b]
            if exact:
                assert flat[level, b] == want, (level, b, flat[level, b], want)
                continue
            bound = (len(values) - 1) * 2.0 ** -53 * math.fsum(abs(v) for v in values) + \
                0.5 * float(np.spacing(abs(want)))
            error = abs(float(flat[level, b]) - want)
            assert error <= bound, (level, b, len(values), error, bound)
            worst = max(worst, error / bound)
    empty = flat[~seen]
    assert not empty.any() and not np.signbit(empty).any()
    return worst
