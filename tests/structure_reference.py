"""The definition of the structure functions ("Structure functions") in numpy, every
operation on its own: numpy's elementwise +, -, * and sqrt are single correctly rounded float64
operations and nothing is fused, so the terms of a pair are the kernel's by bits; the sums are
math.fsum of the terms, correctly rounded, which the kernel's sums may differ from by the
a-priori bound of adding n non-negative terms in any order.

Grids are [nz, ny, nx]; a lag is (lx, ly, lz); a direction (ux, uy, uz)."""
import math

import numpy as np

U = 2.0 ** -53


def pair_indices(shape, lag, periodic):
    """(centre, partner, outside): the flat indices of the centres that have a partner, of their
    partners, and the number of centres without one.  With periodic every axis wraps once."""
    nz, ny, nx = shape
    lx, ly, lz = (int(v) for v in lag)
    assert abs(lx) < nx and abs(ly) < ny and abs(lz) < nz and (lx or ly or lz)
    k, j, i = np.indices(shape, dtype=np.int64)
    qi, qj, qk = i + lx, j + ly, k + lz
    if periodic:
        qi, qj, qk = qi % nx, qj % ny, qk % nz
        inside = np.ones(shape, dtype=bool)
    else:
        inside = (0 <= qi) & (qi < nx) & (0 <= qj) & (qj < ny) & (0 <= qk) & (qk < nz)
    centre = (i + nx * (j + ny * k))[inside]
    partner = (qi + nx * (qj + ny * qk))[inside]
    return centre, partner, int(inside.size - inside.sum())


def pair_terms(components, lag, direction, max_order, periodic):
    """(terms float64 [K, max_order, pairs], pairs, outside, nonfinite) of one lag, the pairs in
    the order of their centres: terms[kind, p - 1] holds w_p of every pair that counts."""
    flat = [np.ascontiguousarray(c, dtype=np.float64).reshape(-1) for c in components]
    centre, partner, outside = pair_indices(components[0].shape, lag, periodic)
    with np.errstate(all="ignore"):
        delta = [v[partner] - v[centre] for v in flat]
        if len(flat) == 1:
            amounts = [np.abs(delta[0])]
            finite = np.isfinite(amounts[0])
        else:
            dx, dy, dz = delta
            ux, uy, uz = (np.float64(v) for v in direction)
            m2 = dx * dx + dy * dy
            m2 = m2 + dz * dz
            along = dx * ux + dy * uy
            along = along + dz * uz
            tx = dx - along * ux
            ty = dy - along * uy
            tz = dz - along * uz
            t2 = tx * tx + ty * ty
            t2 = t2 + tz * tz
            amounts = [np.abs(along), np.sqrt(t2), np.sqrt(m2)]
            finite = np.isfinite(m2)
        terms = np.empty((len(amounts), max_order, int(finite.sum())), dtype=np.float64)
        for kind, amount in enumerate(amounts):
            a = amount[finite]
            w = a
            for p in range(max_order):
                if p > 0:
                    w = w * a
                terms[kind, p] = w
    return terms, int(finite.sum()), outside, int(finite.size - finite.sum())


def structure_functions(components, lags, directions=None, max_order=6, periodic=False):
    """(pairs int64 [M], sums float64 [M, K, max_order], (outside, nonfinite), terms): sums are
    math.fsum of terms[m][kind, p - 1], the list of every lag's pair_terms."""
    components = list(components)
    lags = np.asarray(lags, dtype=np.int64).reshape(-1, 3)
    kinds = len(components)
    assert kinds in (1, 3) and (directions is not None) == (kinds == 3)
    pairs = np.zeros(len(lags), dtype=np.int64)
    sums = np.zeros((len(lags), kinds, max_order), dtype=np.float64)
    outside = nonfinite = 0
    terms = []
    for m, lag in enumerate(lags):
        one, pairs[m], out, bad = pair_terms(
            components, lag, None if directions is None else directions[m], max_order, periodic)
        outside, nonfinite = outside + out, nonfinite + bad
        for kind in range(kinds):
            for p in range(max_order):
                sums[m, kind, p] = math.fsum(one[kind, p])
        terms.append(one)
    return pairs, sums, (outside, nonfinite), terms


def bound(n, total, had=0.0):
    """How far a sum of n non-negative terms added in any order may lie from their math.fsum
    `total`: (n - 1) roundings of the additions and the one of fsum, each at most 2^-53 of the
    sum -- and, where the sum was added to a value `had` the output held, one more of the two
    together."""
    return (max(n - 1, 0) + 1) * U * total + (U * (total + abs(had)) if had else 0.0)
