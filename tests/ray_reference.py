"""The reference of the rays ("Rays"): the definition applied literally, in Python
floats (IEEE binary64: +, -, *, / and math.sqrt are correctly rounded, nothing is fused) on a
plotfile's own level arrays, as write_plotfile takes them.

Per loaded level the leaf mask and leaf values of gradient_reference.leaf_arrays.  A cell is located
by asking every level's leaf mask, finest first: no locator, no box list.  The rays are walked one
after the other in a plain loop.
"""
import math

import numpy as np

from gradient_reference import leaf_arrays

COMPLETE, MISS, TRUNCATED, INVALID = 0, 1, 2, 3


def _floor_clamped(q, lo, hi):
    """floor(q) within [lo, hi]; lo for a q that is not finite."""
    if not math.isfinite(q):
        return lo
    f = math.floor(q)
    return lo if f < lo else (hi if f > hi else f)


class Hierarchy:
    """levels, ref_ratio: as write_plotfile takes them; component: the field's index; sizes[l] =
    (dx, dy, dz); the loaded levels are min_level .. max_level."""

    def __init__(self, levels, ref_ratio, component, sizes, prob_lo, min_level=0, max_level=-1):
        arrays, self.max_level = leaf_arrays(levels, ref_ratio, component, min_level, max_level)
        self.n_levels = self.max_level + 1
        self.origin = [[int(v) for v in arrays[l][0]] for l in range(self.n_levels)]
        self.mask = [arrays[l][1] for l in range(self.n_levels)]
        self.values = [arrays[l][2] for l in range(self.n_levels)]
        self.ratio = [int(r) for r in ref_ratio]
        self.dx = [[float(v) for v in sizes[l]] for l in range(self.n_levels)]
        self.prob_lo = [float(v) for v in prob_lo]
        # [Blo, Bhi]: every leaf mapped to level 0 by floor division
        self.blo = self.bhi = None
        for l in range(self.n_levels):
            k, j, i = np.nonzero(self.mask[l])
            if not k.size:
                continue
            lo = [int(a.min()) + self.origin[l][d] for d, a in enumerate((i, j, k))]
            hi = [int(a.max()) + self.origin[l][d] for d, a in enumerate((i, j, k))]
            for m in range(l, 0, -1):
                lo = [v // self.ratio[m - 1] for v in lo]
                hi = [v // self.ratio[m - 1] for v in hi]
            self.blo = lo if self.blo is None else [min(a, b) for a, b in zip(self.blo, lo)]
            self.bhi = hi if self.bhi is None else [max(a, b) for a, b in zip(self.bhi, hi)]

    def leaf(self, level, index):
        """Whether the level-`level` index is a leaf, and where in the level's arrays."""
        rel = [index[d] - self.origin[level][d] for d in range(3)]
        shape = self.mask[level].shape
        if not (0 <= rel[0] < shape[2] and 0 <= rel[1] < shape[1] and 0 <= rel[2] < shape[0]):
            return False, None
        at = (rel[2], rel[1], rel[0])
        return bool(self.mask[level][at]), at

    def plane(self, level, d, g):
        """X(l, d, g)"""
        return self.prob_lo[d] + float(g) * self.dx[level][d]

    def candidate(self, c, g, p, m):
        if m <= c:
            out = list(g)
            for k in range(c, m, -1):
                out = [v // self.ratio[k - 1] for v in out]
            return out
        refine = 1
        for k in range(c, m):
            refine *= self.ratio[k]
        return [_floor_clamped((p[d] - self.prob_lo[d]) / self.dx[m][d], g[d] * refine,
                               (g[d] + 1) * refine - 1) for d in range(3)]

    def locate(self, c, g, p):
        """Locate(c, G, P) -> (geometry level, index, recorded level, value)."""
        for m in range(self.n_levels - 1, -1, -1):
            cand = self.candidate(c, g, p, m)
            hit, at = self.leaf(m, cand)
            if hit:
                return m, cand, m, float(self.values[m][at])
        finest = self.n_levels - 1
        return finest, self.candidate(c, g, p, finest), -1, math.nan

    def walk(self, a, b, max_trips):
        """One ray -> (status, t_enter, t_leave, segments [(t0, t1, level, value)], integral,
        covered, trips made)."""
        a, b = [float(v) for v in a], [float(v) for v in b]
        nothing = (math.nan, math.nan, [], 0.0, 0.0, 0)
        if not all(math.isfinite(v) for v in a + b):
            return (INVALID,) + nothing
        dirs = [b[d] - a[d] for d in range(3)]
        if all(v == 0.0 for v in dirs):
            return (INVALID,) + nothing
        if self.blo is None:
            return (MISS,) + nothing
        t_enter, t_leave, miss = 0.0, 1.0, False
        for d in range(3):
            lo, hi = self.blo[d], self.bhi[d] + 1
            if dirs[d] == 0.0:
                if not (self.plane(0, d, lo) <= a[d] < self.plane(0, d, hi)):
                    miss = True
                continue
            near, far = (lo, hi) if dirs[d] > 0.0 else (hi, lo)
            t_near = (self.plane(0, d, near) - a[d]) / dirs[d]
            t_far = (self.plane(0, d, far) - a[d]) / dirs[d]
            t_enter = t_near if t_near > t_enter else t_enter
            t_leave = t_far if t_far < t_leave else t_leave
        if miss or not t_enter < t_leave:
            return (MISS,) + nothing
        length = math.sqrt((dirs[0] * dirs[0] + dirs[1] * dirs[1]) + dirs[2] * dirs[2])
        t_cur = t_enter
        p = [a[d] + t_cur * dirs[d] for d in range(3)]
        g = [_floor_clamped((p[d] - self.prob_lo[d]) / self.dx[0][d], self.blo[d], self.bhi[d])
             for d in range(3)]
        c = 0
        segments, integral, covered, status, trips = [], 0.0, 0.0, TRUNCATED, 0
        for _ in range(max_trips):
            trips += 1
            l, g, level, value = self.locate(c, g, p)
            t_out, exit_axis = None, -1
            for d in range(3):
                if dirs[d] == 0.0:
                    continue
                far = g[d] + 1 if dirs[d] > 0.0 else g[d]
                t = (self.plane(l, d, far) - a[d]) / dirs[d]
                if exit_axis < 0 or t < t_out:
                    t_out, exit_axis = t, d
            ahead = t_out if t_out > t_cur else t_cur
            t_next = ahead if ahead < t_leave else t_leave
            if t_next > t_cur:
                segments.append((t_cur, t_next, level, value))
                if level >= 0:
                    w = (t_next - t_cur) * length
                    covered = covered + w
                    if math.isfinite(value):
                        integral = integral + value * w
            if not t_out < t_leave:
                status = COMPLETE
                break
            g = list(g)
            g[exit_axis] += 1 if dirs[exit_axis] > 0.0 else -1
            z = list(g)
            for m in range(l, 0, -1):
                z = [v // self.ratio[m - 1] for v in z]
            if any(z[d] < self.blo[d] or z[d] > self.bhi[d] for d in range(3)):
                status = COMPLETE
                break
            p = [a[d] + t_next * dirs[d] for d in range(3)]
            c, t_cur = l, t_next
        return status, t_enter, t_leave, segments, integral, covered, trips

    def rays(self, start, end, max_trips):
        """Returns a dict of arrays shaped as api.ray_scene's: offsets, status, t_enter, t_leave,
        integral, covered per ray; t0, t1, level, value per segment; and trips int64 [n], the
        trips every ray made."""
        start = np.ascontiguousarray(start, dtype=np.float64).reshape(-1, 3)
        end = np.ascontiguousarray(end, dtype=np.float64).reshape(-1, 3)
        n = start.shape[0]
        out = {"status": np.zeros(n, dtype=np.uint8), "t_enter": np.zeros(n), "t_leave": np.zeros(n),
               "integral": np.zeros(n), "covered": np.zeros(n),
               "trips": np.zeros(n, dtype=np.int64)}
        offsets, segments = [0], []
        for s in range(n):
            status, t_enter, t_leave, found, integral, covered, trips = self.walk(
                start[s], end[s], max_trips)
            out["trips"][s] = trips
            out["status"][s], out["t_enter"][s], out["t_leave"][s] = status, t_enter, t_leave
            out["integral"][s], out["covered"][s] = integral, covered
            segments += found
            offsets.append(len(segments))
        out["offsets"] = np.array(offsets, dtype=np.int64)
        out["t0"] = np.array([s[0] for s in segments], dtype=np.float64)
        out["t1"] = np.array([s[1] for s in segments], dtype=np.float64)
        out["level"] = np.array([s[2] for s in segments], dtype=np.int8)
        out["value"] = np.array([s[3] for s in segments], dtype=np.float64)
        return out

    def default_max_trips(self):
        """8 + 2 sum_d (Bhi[d] - Blo[d] + 1) (r_0 ... r_(n_levels - 2))"""
        if self.blo is None:
            return 8
        refine = 1
        for r in self.ratio[:self.n_levels - 1]:
            refine *= r
        return 8 + 2 * sum(h - l + 1 for l, h in zip(self.blo, self.bhi)) * refine


def rays(levels, ref_ratio, component, sizes, prob_lo, start, end, max_trips=None, min_level=0,
         max_level=-1):
    hierarchy = Hierarchy(levels, ref_ratio, component, sizes, prob_lo, min_level, max_level)
    return hierarchy.rays(start, end,
                          hierarchy.default_max_trips() if max_trips is None else max_trips)
