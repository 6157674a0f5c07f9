"""The reference of the clump binding ("Clump binding"): the members of the wanted
clumps by a literal loop over the scene's cells, the self-energy by math.fsum over the pairs'
terms, and M, K and T by math.fsum over the members.  Plain Python and numpy on a plotfile's own
level arrays, as write_plotfile takes them, and on the per-level label arrays of
clump_reference.clump_levels.
"""
import math

import numpy as np

from gradient_reference import leaf_arrays

U = 2.0 ** -53


def members(labels, n, wanted, levels, ref_ratio, scene_boxes, prob_lo, sizes, components=()):
    """The canonical member list of the clumps c with wanted[c - 1]: every cell of the scene boxes
    (level, lo, hi), in scene order and then k, j, i -- which numbers the ordinals --, whose label is
    such a c, sorted by (c - 1, ordinal).  Returns a dict: keys (c - 1) << 32 | ordinal (python
    ints), labels (the wanted c, ascending), offsets, ordinal, level, centres [m, 3] = prob_lo +
    (f64(I) + 0.5) * dx_l with I the cell's index in its level, values {component: [m]} raw."""
    fields = {f: leaf_arrays(levels, ref_ratio, f)[0] for f in components}
    found = []
    ordinal = 0
    for level, lo, hi in scene_boxes:
        dlo = levels[level]["domain"][0]
        for k in range(lo[2], hi[2] + 1):
            for j in range(lo[1], hi[1] + 1):
                for i in range(lo[0], hi[0] + 1):
                    at = (k - dlo[2], j - dlo[1], i - dlo[0])
                    label = float(labels[level][at])
                    if label != 0.0:
                        c = int(label)
                        assert 1 <= c <= n and c == label
                        if wanted[c - 1]:
                            centre = [prob_lo[a] + (float(index) + 0.5) * sizes[level][a]
                                      for a, index in enumerate((i, j, k))]
                            found.append((c - 1, ordinal, level, centre,
                                          [float(fields[f][level][2][at]) for f in components]))
                    ordinal += 1
    found.sort(key=lambda member: (member[0], member[1]))
    wanted_labels = [c + 1 for c in range(n) if wanted[c]]
    counts = [sum(1 for member in found if member[0] == c - 1) for c in wanted_labels]
    return {"keys": [(c << 32) | o for c, o, _, _, _ in found],
            "labels": np.array(wanted_labels, dtype=np.int64),
            "offsets": np.concatenate([[0], np.cumsum(counts)]).astype(np.int64),
            "ordinal": np.array([o for _, o, _, _, _ in found], dtype=np.int64),
            "level": np.array([l for _, _, l, _, _ in found], dtype=np.uint8),
            "centres": np.array([x for _, _, _, x, _ in found], dtype=np.float64).reshape(-1, 3),
            "values": {f: np.array([v[q] for _, _, _, _, v in found], dtype=np.float64)
                       for q, f in enumerate(components)}}


def self_energy_literal(x, y, z, m):
    """W = sum_{i<j} m_i m_j / r_ij, pair by pair in Python floats (IEEE binary64, nothing fused),
    the terms added exactly by math.fsum and rounded once."""
    terms = []
    for i in range(len(m)):
        for j in range(i + 1, len(m)):
            dx, dy, dz = x[i] - x[j], y[i] - y[j], z[i] - z[j]
            terms.append(m[i] * m[j] / math.sqrt((dx * dx + dy * dy) + dz * dz))
    return math.fsum(terms)


def self_energy(x, y, z, m):
    """The same terms, a row of numpy operations per member i -- correctly rounded like Python's --
    and math.fsum per row and over the rows' sums: two roundings of sums of terms that are not
    negative, so within 2 * 2^-53 of the exact sum of the terms (self_energy_literal rounds it
    once).  For segments too long for the pair loop."""
    x, y, z, m = (np.asarray(a, dtype=np.float64) for a in (x, y, z, m))
    rows = []
    for i in range(len(m) - 1):
        dx, dy, dz = x[i] - x[i + 1:], y[i] - y[i + 1:], z[i] - z[i + 1:]
        rows.append(math.fsum((m[i] * m[i + 1:] / np.sqrt((dx * dx + dy * dy) + dz * dz)).tolist()))
    return math.fsum(rows)


def segment_energies(x, y, z, m, offsets):
    return np.array([self_energy(*(a[offsets[s]:offsets[s + 1]] for a in (x, y, z, m)))
                     for s in range(len(offsets) - 1)], dtype=np.float64)


def binding(level, rho, volumes, velocity=None, e=None):
    """One clump's members -> a dict: m per member (rho * vol_l; 0 where rho is negative or not
    finite, and such a member's velocity is not looked at), excluded, M, K, T by math.fsum, nonfinite, and what bounds a sum of the same terms
    added in any order: abs_M, abs_T (sum |terms|), n, and for K the parts of k_tolerance."""
    vol = np.array([volumes[l] for l in level], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        usable = np.isfinite(rho) & (rho >= 0.0)
    m = np.where(usable, rho * vol, 0.0)
    out = {"m": m, "excluded": int((~usable).sum()), "n": len(m), "M": math.fsum(m.tolist()),
           "K": 0.0, "T": 0.0, "nonfinite": 0, "k_tolerance": 0.0}
    out["abs_M"] = out["M"]
    n, M = len(m), out["M"]
    if velocity is not None and M > 0.0:
        total, tolerance = [], 0.0
        for v in velocity:
            v = np.where(m > 0.0, v, 0.0)           # a member without mass has no velocity
            momentum = (m * v).tolist()
            vbar = math.fsum(momentum) / M
            away = v - vbar
            terms = m * (away * away)
            S = math.fsum(terms.tolist())
            total.append(S)
            # another order of additions, in the momentum and in M, moves vbar by at most e, which
            # moves a term by at most m (2 |away| e + e^2) besides its own three roundings; then
            # n - 1 additions
            e_bar = (2 * n + 2) * U * math.fsum(abs(t) for t in momentum) / M
            tolerance += (n + 4) * U * S + 2.0 * e_bar * math.fsum((m * np.abs(away)).tolist()) \
                + M * e_bar * e_bar
        out["K"] = 0.5 * math.fsum(total)
        out["k_tolerance"] = 0.5 * tolerance + 4 * U * out["K"]
    if e is not None:
        known = np.isfinite(e)
        terms = np.where(known, e * vol, 0.0)
        out["T"] = math.fsum(terms.tolist())
        out["abs_T"] = math.fsum(np.abs(terms).tolist())
        out["nonfinite"] = int((~known).sum())
    else:
        out["abs_T"] = 0.0
    return out
