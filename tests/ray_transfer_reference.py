"""The reference of ray transfer ("Ray transfer").  It walks nothing of its own:
ray_reference.Hierarchy.rays lists the segments of the source function S, the opacity a, the bin
field g and the width s, the lists must agree in everything but the values
(ray_sums_reference.same_geometry), and the definition is formed from the segments in Python floats
(IEEE binary64, nothing fused), in walk order, with math.expm1, math.exp and math.erf:

    dtau   = ((a * w) * share) * rdv[c]
    I[c]   = I[c] + (S * (-expm1(-dtau))) * exp(-tau[c])          tau[c] before this segment
    tau[c] = tau[c] + dtau

It also returns, per ray and channel, the a-priori bounds the device is held to, from its own
values, with u = 2^-53 and the ulp figures of OpenCL's full profile (exp 3, expm1 3, erf 16):

  intensity, every form   (2 n + 24) u sum |term_i| + (n + 1) 2^-1022, n the segments of the
                          channel whose dtau is not 0
  tau, broadened          u ((2 n + 4) tau + 22 rdv[c] sum a_i w_i)
  intensity, broadened    the above plus u sum_i (|S_i| T_i (22 a_i w_i rdv[c] + 4 dtau_i)
                                                 + |term_i| (22 A_i rdv[c] + (2 i + 4) tau_i))

In the two broadened sums i runs over the counted segments of the ray whose share the error
function gave (s > 0), whether or not this reference's share of the channel is 0: the device's erf
may differ from math.erf by 16 ulp at either edge, so a share that is exactly 0 here need not be 0
there; T_i = exp(-tau_i), tau_i the channel's optical depth in front of segment i, A_i the sum of
a w over the earlier such segments.  tau, outside, counted and covered of the grey and the sharp
form are plain IEEE sums and are compared by bits."""
import bisect
import math

import numpy as np

from ray_sums_reference import same_geometry

U = 2.0 ** -53
RSQRT2 = 0.70710678118654752440
TINY = 2.0 ** -1022


def reciprocal_widths(edges):
    """rdv[c] = 1.0 / (edges[c + 1] - edges[c]) in Python floats."""
    e = [float(v) for v in edges]
    return [1.0 / (e[c + 1] - e[c]) for c in range(len(e) - 1)]


def clamped_erf(a):
    return -1.0 if a <= -6.0 else (1.0 if a >= 6.0 else math.erf(a))


def shares_of(edges, g, s):
    """([(channel, share)] with share != 0, share under, share over) of a counted cell."""
    nc = len(edges) - 1
    if s == 0.0:
        if g < edges[0]:
            return [], 1.0, 0.0
        if g > edges[nc]:
            return [], 0.0, 1.0
        c = min(bisect.bisect_right(edges, g) - 1, nc - 1)     # the last channel closed at the top
        return [(c, 1.0)], 0.0, 0.0
    q = [clamped_erf(((edge - g) / s) * RSQRT2) for edge in edges]
    shares = []
    for c in range(nc):
        share = 0.5 * (q[c + 1] - q[c])
        if share != 0.0:
            shares.append((c, share))
    return shares, 0.5 * (q[0] + 1.0), 0.5 * (1.0 - q[nc])


def transfer_of(start, end, source, opacity, bin_field=None, width=None, edges=None):
    """source, opacity, bin_field (or None: grey), width (or None): what Hierarchy.rays returned
    for start -> end through each field.  Returns a dict of arrays: per ray count uint32, status
    uint8, t_enter, t_leave, counted, covered; intensity, tau [nc, n]; outside [2, n] (None for
    grey); intensity_bound, tau_bound [nc, n] (tau_bound is 0 unless a width is given); abs_terms
    [nc, n] = sum |term_i|; segments [nc, n] the n of the bounds; opacity_sum [n] = sum a w over the
    counted segments."""
    start = np.ascontiguousarray(start, dtype=np.float64).reshape(-1, 3)
    end = np.ascontiguousarray(end, dtype=np.float64).reshape(-1, 3)
    n = start.shape[0]
    assert source["offsets"].size == n + 1
    assert width is None or bin_field is not None
    assert (bin_field is None) == (edges is None)
    for other in (opacity, bin_field, width):
        assert other is None or same_geometry(source, other), \
            "the fields were walked through other cells"
    if edges is None:
        e, rdv, nc = None, [1.0], 1
    else:
        e = [float(v) for v in edges]
        rdv, nc = reciprocal_widths(e), len(e) - 1
    offsets = source["offsets"]
    out = {"count": np.diff(offsets).astype(np.uint32), "status": source["status"].copy(),
           "t_enter": source["t_enter"].copy(), "t_leave": source["t_leave"].copy(),
           "counted": np.zeros(n), "covered": np.zeros(n), "opacity_sum": np.zeros(n),
           "intensity": np.zeros((nc, n)), "tau": np.zeros((nc, n)),
           "outside": None if e is None else np.zeros((2, n)),
           "intensity_bound": np.zeros((nc, n)), "tau_bound": np.zeros((nc, n)),
           "abs_terms": np.zeros((nc, n)), "segments": np.zeros((nc, n), np.int64)}
    for r in range(n):
        d = [float(end[r, k]) - float(start[r, k]) for k in range(3)]
        square = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
        length = math.sqrt(square) if math.isfinite(square) else math.nan
        counted = covered = under = over = 0.0
        intensity, tau = [0.0] * nc, [0.0] * nc
        abs_terms, segments = [0.0] * nc, [0] * nc
        extra = [0.0] * nc        # the broadened intensity bound's sum, without its u
        spread = 0.0              # A: sum a w over the segments with s > 0 so far
        spread_index = 0          # ... and how many they are
        total = 0.0
        for i in range(int(offsets[r]), int(offsets[r + 1])):
            if int(source["level"][i]) < 0:
                continue
            w = (float(source["t1"][i]) - float(source["t0"][i])) * length
            covered = covered + w
            S, a = float(source["value"][i]), float(opacity["value"][i])
            counts = math.isfinite(S) and math.isfinite(a) and a >= 0.0
            g = s = 0.0
            if bin_field is not None:
                g = float(bin_field["value"][i])
                counts = counts and math.isfinite(g)
            if width is not None:
                s = float(width["value"][i])
                counts = counts and math.isfinite(s) and s >= 0.0
            if not counts:
                continue
            counted = counted + w
            aw = a * w
            total = total + aw
            if e is None:
                shares, share_under, share_over = [(0, 1.0)], 0.0, 0.0
            else:
                shares, share_under, share_over = shares_of(e, g, s)
                under = under + aw * share_under
                over = over + aw * share_over
            broadened = s > 0.0
            if broadened:
                spread_index += 1
            for c, share in shares:
                dtau = (aw * share) * rdv[c]
                transmitted = math.exp(-tau[c])
                term = (S * (-math.expm1(-dtau))) * transmitted
                if dtau != 0.0:
                    segments[c] += 1
                abs_terms[c] += abs(term)
                if broadened:
                    extra[c] += abs(S) * transmitted * (22.0 * aw * rdv[c] + 4.0 * abs(dtau)) + \
                        abs(term) * (22.0 * spread * rdv[c] + (2 * spread_index + 4) * tau[c])
                intensity[c] = intensity[c] + term
                tau[c] = tau[c] + dtau
            if broadened:
                # a share that is 0 here may not be 0 on the device: its own dtau's part
                hit = {c for c, _ in shares}
                for c in range(nc):
                    if c not in hit:
                        extra[c] += abs(S) * math.exp(-tau[c]) * (22.0 * aw * rdv[c])
                spread = spread + aw
        out["counted"][r], out["covered"][r], out["opacity_sum"][r] = counted, covered, total
        if e is not None:
            out["outside"][0, r], out["outside"][1, r] = under, over
        for c in range(nc):
            out["intensity"][c, r], out["tau"][c, r] = intensity[c], tau[c]
            out["abs_terms"][c, r], out["segments"][c, r] = abs_terms[c], segments[c]
            m = segments[c]
            bound = (2 * m + 24) * U * abs_terms[c] + (m + 1) * TINY
            if width is not None:
                bound += U * extra[c]
                out["tau_bound"][c, r] = U * ((2 * m + 4) * tau[c] + 22.0 * rdv[c] * spread)
            out["intensity_bound"][c, r] = bound
    return out


def ray_transfer(start, end, source, opacity, bin_field=None, width=None, edges=None,
                 max_trips=None):
    """source, opacity, bin_field, width: ray_reference.Hierarchy of the fields over the same
    levels (the last two may be None)."""
    if max_trips is None:
        max_trips = source.default_max_trips()
    walked = [None if h is None else h.rays(start, end, max_trips)
              for h in (source, opacity, bin_field, width)]
    return transfer_of(start, end, *walked, edges=edges)
