"""The reference of the streamlines ("Streamlines"): plain numpy on a plotfile's own
level arrays, as write_plotfile takes them, applying the definition literally.

Per loaded level the leaf mask and leaf values of gradient_reference.leaf_arrays, one set per field
over the same leaves.  A point is located by asking every level's leaf mask, finest first: no
locator, no box list.  The seeds advance side by side as numpy arrays; every operation on them is
an elementwise IEEE binary64 one (+, -, *, /, sqrt, floor), written in the order the definition
gives, so a lane's numbers are those of numpy scalars.
"""
import numpy as np

from gradient_reference import leaf_arrays

LIMIT = np.float64(2.0 ** 30)
REACHED, OUTSIDE, STAGNANT, NONFINITE = 0, 1, 2, 3


class Hierarchy:
    """levels, ref_ratio: as write_plotfile takes them; components: the indices of vx, vy, vz and,
    if sample is not None, of the sample field; sizes[l] = (dx, dy, dz); the loaded levels are
    min_level .. max_level."""

    def __init__(self, levels, ref_ratio, components, sizes, prob_lo, min_level=0, max_level=-1,
                 sample=None):
        fields = list(components) + ([sample] if sample is not None else [])
        per_field = [leaf_arrays(levels, ref_ratio, c, min_level, max_level) for c in fields]
        self.max_level = per_field[0][1]
        first = per_field[0][0]
        self.origin = [first[l][0] for l in range(self.max_level + 1)]
        self.mask = [first[l][1] for l in range(self.max_level + 1)]
        # values[l]: [fields, nz, ny, nx]
        self.values = [np.stack([arrays[l][2] for arrays, _ in per_field])
                       for l in range(self.max_level + 1)]
        self.ratio = list(ref_ratio)
        self.dx = [np.array(sizes[l], dtype=np.float64) for l in range(self.max_level + 1)]
        self.prob_lo = np.array(prob_lo, dtype=np.float64)
        self.has_sample = sample is not None

    def leaf(self, level, index):
        """index [n, 3] of `level` -> (is a leaf [n], where in the level's arrays)."""
        rel = index - self.origin[level][None, :]
        extent = np.array(self.mask[level].shape[::-1], dtype=np.int64)
        inside = np.all((rel >= 0) & (rel < extent[None, :]), axis=1)
        safe = np.where(inside[:, None], rel, 0)
        at = (safe[:, 2], safe[:, 1], safe[:, 0])
        return inside & self.mask[level][at], at

    def locate(self, points):
        """points [n, 3] -> (leaf level [n], -1 outside; q [n, 3] at that level; G [n, 3])."""
        n = points.shape[0]
        level = np.full(n, -1, dtype=np.int64)
        q = np.zeros((n, 3))
        index = np.zeros((n, 3), dtype=np.int64)
        open_ = np.ones(n, dtype=bool)                  # neither found nor outside yet
        for l in range(self.max_level, -1, -1):
            with np.errstate(all="ignore"):
                at = (points - self.prob_lo[None, :]) / self.dx[l][None, :]
            bad = ~(np.isfinite(at) & (at >= -LIMIT) & (at < LIMIT)).all(axis=1)
            open_ &= ~bad                               # outside for good
            cell = np.floor(np.where(bad[:, None], 0.0, at)).astype(np.int64)
            hit = self.leaf(l, cell)[0] & open_
            level[hit], q[hit], index[hit] = l, at[hit], cell[hit]
            open_ &= ~hit
        return level, q, index

    def corner(self, level, index):
        """The corner rule for the level-`level` indices index [n, 3]: (present [n], values
        [fields, n])."""
        n = index.shape[0]
        present = np.zeros(n, dtype=bool)
        values = np.zeros((self.values[0].shape[0], n))
        mapped = index.copy()
        for m in range(level, -1, -1):
            if m < level:
                mapped = mapped // self.ratio[m]        # floors, also below zero
            hit, at = self.leaf(m, mapped)
            take = hit & ~present
            values[:, take] = self.values[m][(slice(None),) + at][:, take]
            present |= hit
        return present, values

    def evaluate(self, points):
        """points [n, 3] -> dict: leaf [n] (bool), level [n], finite [n] (the velocity), v [n, 3]
        and sample [n] (the leaf's or the trilinear value; only with a sample field)."""
        n = points.shape[0]
        level, q, index = self.locate(points)
        fields = self.values[0].shape[0]
        out = {"leaf": level >= 0, "level": level, "finite": np.zeros(n, dtype=bool),
               "v": np.zeros((n, 3)), "sample": np.zeros(n)}
        for l in range(self.max_level + 1):
            pick = np.nonzero(level == l)[0]
            if not pick.size:
                continue
            u = q[pick] - 0.5
            low = np.floor(u)
            base = low.astype(np.int64)
            w = u - base.astype(np.float64)
            present = np.ones(pick.size, dtype=bool)
            corners = np.zeros((8, fields, pick.size))
            for c in range(8):
                step = np.array([c & 1, (c >> 1) & 1, c >> 2], dtype=np.int64)
                there, corners[c] = self.corner(l, base + step[None, :])
                present &= there
            is_leaf, at = self.leaf(l, index[pick])
            assert is_leaf.all()
            own = self.values[l][(slice(None),) + at]                   # [fields, n]
            with np.errstate(all="ignore"):
                ax = [corners[2 * e] + w[None, :, 0] * (corners[2 * e + 1] - corners[2 * e])
                      for e in range(4)]                                 # (dj, dk) = 00 10 01 11
                ay = [ax[0] + w[None, :, 1] * (ax[1] - ax[0]), ax[2] + w[None, :, 1] * (ax[3] - ax[2])]
                smooth_value = ay[0] + w[None, :, 2] * (ay[1] - ay[0])   # [fields, n]
            finite = np.isfinite(corners)                                # [8, fields, n]
            smooth = present & finite[:, :3].all(axis=(0, 1))            # one decision for V
            v = np.where(smooth[None, :], smooth_value[:3], own[:3])
            out["v"][pick] = v.T
            out["finite"][pick] = smooth | np.isfinite(own[:3]).all(axis=0)
            if self.has_sample:
                smooth_sample = present & finite[:, 3].all(axis=0)
                out["sample"][pick] = np.where(smooth_sample, smooth_value[3], own[3])
        return out

    def trace(self, seeds, step, direction, max_steps):
        """Returns a dict: points [n, max_steps + 1, 3] (NaN past a line's count), counts [n],
        status uint8 [n], samples [n, max_steps + 1] (NaN past the count) or None."""
        seeds = np.ascontiguousarray(seeds, dtype=np.float64).reshape(-1, 3)
        n = seeds.shape[0]
        step, direction = np.float64(step), np.float64(direction)
        points = np.full((n, max_steps + 1, 3), np.nan)
        samples = np.full((n, max_steps + 1), np.nan) if self.has_sample else None
        counts = np.zeros(n, dtype=np.int64)
        status = np.full(n, REACHED, dtype=np.uint8)
        alive = np.arange(n)                                             # the lines still going
        p = seeds.copy()
        for number in range(max_steps + 1):
            if not alive.size:
                break
            e = self.evaluate(p[alive])
            if number == 0:                                              # a seed outside: no point
                status[alive[~e["leaf"]]] = OUTSIDE
                keep = e["leaf"]
                alive, e = alive[keep], {k: v[keep] for k, v in e.items()}
            points[alive, number] = p[alive]
            if samples is not None:
                samples[alive, number] = np.where(e["leaf"], e["sample"], np.nan)
            counts[alive] = number + 1
            if number == max_steps:
                break
            # the four stages; a line ends at the first that fails
            h = np.zeros(alive.size)
            has_level = e["level"] >= 0
            for l in range(self.max_level + 1):
                h[e["level"] == l] = step * min(min(self.dx[l][0], self.dx[l][1]), self.dx[l][2])
            going = np.ones(alive.size, dtype=bool)
            k = np.zeros((alive.size, 3))
            total = np.zeros((alive.size, 3))
            for stage in range(4):
                if stage > 0:
                    reach = h if stage == 3 else 0.5 * h
                    with np.errstate(all="ignore"):
                        at = p[alive] + reach[:, None] * k
                    e = self.evaluate(np.where(going[:, None], at, np.nan))
                with np.errstate(all="ignore"):
                    norm = np.sqrt((e["v"][:, 0] * e["v"][:, 0] + e["v"][:, 1] * e["v"][:, 1])
                                   + e["v"][:, 2] * e["v"][:, 2])
                    k = (direction * e["v"]) / norm[:, None]
                failed = np.where(~e["leaf"], OUTSIDE,
                                  np.where(~e["finite"], NONFINITE,
                                           np.where(norm == 0.0, STAGNANT, REACHED)))
                ends = going & (failed != REACHED)
                status[alive[ends]] = failed[ends]
                going &= ~ends
                with np.errstate(all="ignore"):
                    if stage == 0:
                        total = k.copy()
                    elif stage == 3:
                        total = total + k
                    else:
                        total = total + 2.0 * k
            assert has_level[going].all()
            with np.errstate(all="ignore"):
                moved = p[alive] + (h / 6.0)[:, None] * total
            p[alive[going]] = moved[going]
            alive = alive[going]
        return {"points": points, "counts": counts, "status": status, "samples": samples}


def trace(levels, ref_ratio, components, sizes, prob_lo, seeds, step, direction, max_steps,
          min_level=0, max_level=-1, sample=None):
    return Hierarchy(levels, ref_ratio, components, sizes, prob_lo, min_level, max_level,
                     sample).trace(seeds, step, direction, max_steps)


def sample_points(levels, ref_ratio, component, sizes, prob_lo, points, min_level=0, max_level=-1):
    """(value [n], inside [n]) of one field at points, by lines of no steps."""
    out = trace(levels, ref_ratio, (component,) * 3, sizes, prob_lo, points, 1.0, 1, 0, min_level,
                max_level, component)
    return out["samples"][:, 0], out["counts"] == 1
