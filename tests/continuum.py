"""An exact float64 reference of what the ray march samples: the line integrals of a
piecewise-constant field along the pinhole camera's rays (and, given colour tables, the
emission-absorption colour and alpha of the same rays), and the brackets inside which a march
that takes samples every `step` must land.  numpy only, float64 only, no stepping: written from
the definition of the picture, it shares no code and no float32 path with the oracle or the
kernels.

The picture (Common/VolumePainter.cpp:631-656, 737-770; Common/CameraUtils.hpp)
-------------------------------------------------------------------------------
forward f = (look_at - eye) / |look_at - eye|, right r = (f x up) / |f x up|, u = r x f (a
right-handed frame: looking along f with `up` upwards, r points to the right).  The image has
`width` columns x and `height` rows y; ROW 0 IS THE BOTTOM of the scene.  fov_y is the FULL
vertical opening angle.  Pixel (x, y) looks through its CENTRE, along

    D = f + ((2 (x + 1/2) / width  - 1) tan(fov_y / 2) (width / height)) r
          + ((2 (y + 1/2) / height - 1) tan(fov_y / 2)) u,          d = D / |D|,

from the eye: point(t) = eye + t d.  A box is [min_corner, max_corner] with cells[k, j, i] (x
fastest) of size h = (max - min) / (nx, ny, nz); cell (i, j, k) is the half-open brick from
min + (i, j, k) h.  Its step is min(h) / 2, its mesh epsilon 1e-4 |max - min| (:600, :688-692).

Exact quantities
----------------
chords() intersects the ray with the box (slab test) and walks the cells it crosses (the
traversal of Amanatides & Woo, done for all rays at once by merging the three sorted families of
plane crossings instead of stepping from one to the next): segments [t_j, t_j+1], the cell of
each and its chord length l_c.  length = sum l_c over finite cells, column = sum v_c l_c.

What a stepping march may differ by (every margin below is derived here, none is measured)
------------------------------------------------------------------------------------------
u = 2^-24, the unit round-off of float32.

delta, the uncertainty of a float32 sample POSITION against the float64 ray, infinity norm:
    delta = (C_POSITION + k) u (|eye|_inf + t)
k = number of `distance += step` additions made so far in the box (each rounds by <= u t; bounded
by ceil(chord / step) + 1).  C_POSITION counts every other rounding between the camera and the
cell index, each in units of u (|eye|_inf + t) at a point at parameter t (|d| <= 1, |corner|_inf
<= |eye|_inf + t).  Assumed, and true of every camera the tests use: tan(fov_y / 2) x aspect <= 1
(so both plane coordinates are at most 1 in size) and fov_y <= 90 degrees.
  the unit direction d, 49 in all:
    ndc = (x + 1/2) * (1 / W) * 2 - 1: the reciprocal and the product, relative, on a value <= 1,
        doubled by the * 2 (4), the subtraction's own rounding on a result <= 1 (1)  -> 5, absolute
    T = tan(fov * 0.5 * pi / 180): pi as a float, the product, the division (3), carried through
        tan, whose relative condition x / (sin x cos x) is <= pi / 2 up to 45 degrees (-> 5), and
        tan's own result to one ulp (2)                                              -> 7, relative
    aspect = W / H (1); the products ndc * T and * aspect (2)
    plane X: 5 + (7 + 1 + 2) |ndc| <= 15, absolute; plane Y (no aspect, one product less) <= 14
    D_a = f_a + X r_a + Y u_a: X's and Y's errors weighted by r_a and u_a; the casts of f_a, r_a,
        u_a to float32 (3), the two products (2), the two additions (2)
        -> error of D in the 2-norm <= 15 |r| + 14 |u| + 7 sqrt(3) = 15 + 14 + 12.2 <= 42
    d = D / |D|: normalising projects D's error off d and divides it by |D| >= 1, a contraction
        in the 2-norm, which bounds the infinity norm: 42.  The normalisation's own roundings, all
        relative on |d_a| <= 1: |D|^2 from three squares and two additions of positive terms (3,
        halved by the square root: 1.5), rsqrt to one ulp (2), its reciprocal (1), the reciprocal
        of the length (1), the final product (1)                                      -> 6.5 <= 7
  the eye cast to float32                                                                       1
  the box corners cast to float32 (moves a face: the same effect as moving the point)           1
  the slab parameter (corner - origin) * (1 / d_a): subtract, reciprocal, multiply              3
  tmin + meshEpsilon                                                                            1
  origin + d * distance: multiply, add                                                          2
  the cell index (pos - corner) / h: subtract, divide (or reciprocal and multiply: 2), and h
        itself = (max - min) / n: subtract, divide                                              5
  C_POSITION = 49 + 1 + 1 + 3 + 1 + 2 + 5 = 62.
A face perpendicular to axis a is crossed at a parameter uncertain by tau = delta / |d_a|.

Samples sit at s_0 + k step with s_0 = t_entry + meshEpsilon (the phase restarts in every box).
N(t) = #{samples < t} obeys  step N(t) - (t - t_entry)  in  [-eps, step - eps]  for t past s_0.
Let A_j be the number of samples the march attributes to the cells before boundary j, and
E_j = step A_j - (t_j - t_entry).  Its own boundary is uncertain by tau_j and its phase by delta:

    E_j  in  [-(eps + delta + tau_j),  max(step - eps, 0) + delta + tau_j]  =  [-below_j, above_j]

For a per-cell quantity q (q = v: column; q = 1 on finite cells: length), with q = 0 before and
after the box, summation by parts gives

    step sum_samples q - sum_c q_c l_c  =  - sum_j (q_j - q_j-1) E_j

the sum running over the entry (jump q_first), every cell change along the ray and the exit (jump
-q_last).  Each term is bounded on either side by the matching end of E_j's interval, so the
bracket is ONE-SIDED per jump: [exact - under, exact + over].  Summed with absolute values it
reads step (|v_first| + |v_last| + TV) + ..., the safe form; kept per boundary and per sign it is
about half as wide.  At the entry, sharper and proved: no sample lies before s_0, so E_0 = step x
(the number of leading samples the march drops as outside) >= 0; none can be dropped when eps >
tau_0 + delta (the first sample is then certainly inside) and E_0 = 0; otherwise at most
floor((tau_0 + delta - eps) / step) + 1.  For length this gives, per box, over = step - eps +
delta + tau_exit and under = eps + delta + tau_exit (+ step per sample droppable at the entry):
within (step + eps) + 2 delta.
One more term: where a segment's end lies within delta of an edge of its cell (not only of the
face it crosses), samples of that segment may be read from a neighbour off the ray, or dropped as
outside the box.  There are at most l_c / step + 1 of them, each wrong by at most R_c = max(|v_n -
v_c| over the 26 neighbours n, |v_c|): the segment adds (l_c + step) R_c.
step in float32 differs from min(h) / 2 by <= 2 u relative: 2 u (length or column) is added.

Maximum intensity, integers only: a sample certainly falls in segment j when, shrunk by tau at
both ends and started no earlier than s_0 <= t_entry + eps + delta, it is still longer than one
step (any interval of that length holds a sample), and the segment is not near an edge.
    lower = max index over such segments (-1 if none)  <=  MIP  <=
    upper = max index over all crossed cells, each widened to its 3x3x3 neighbourhood when near
            an edge.
Homogeneous medium: n_b = length_got / step is an integer within the length bracket; the pixel's
transmittance lies between prod_b (1 - a_b)^n_b at the two ends.  That bracket is one-sided like
the length's (a march overcounts by half a step per box on average), so the medium's own
transmittance (1 - a_ref)^(length / reference step) is held against the phase-free bracket n_b in
[floor(l_b / step_b), ceil(l_b / step_b)] instead: it falls inside exactly when the per-level
opacities a_b are consistent with a_ref, 1 - a_b = (1 - a_ref)^(step_b / reference step).

Colour: the emission-absorption picture (expected(..., tables=...))
------------------------------------------------------------------
Scope: finite cells, no antialiasing, no wireframe, table colours in [0, 1] and per-sample
opacities a < 1 (asserted; the tests keep a <= 0.6).  Opaque entries (a = 1, kappa infinite) are
out of scope.  The table P_b [256, 4] = (r, g, b, a) of a box's level is INPUT of the march (built
by the product's host functions, which tests/test_host_parity.py pins); box.index holds each
cell's entry.

Along one ray inside box b, with chords()' boundaries t_0 .. t_m and entries k_0 .. k_m-1, write
(c_j, a_j) = P_b[k_j], kappa_j = -log1p(-a_j) and Y_j = (t_j - t_0) / step_b, the boundaries
measured in samples.  The layer and the alpha of the box are

    L_b = sum_j T_<j c_j (1 - (1 - a_j)^(Y_j+1 - Y_j)),   A_b = 1 - prod_j (1 - a_j)^(Y_j+1 - Y_j),

T_<j the product over the segments before j, and the pixel is sum_b (prod_b' before b (1 - A_b'))
L_b, the (disjoint) boxes in the order of their entries along the ray: premultiplied colour, as
the march stores it.  At integer Y this is exactly the recurrence alpha = a (1 - A); C += c alpha;
A += alpha.  At the exact real Y it is the reference value `colour`; alpha = 1 - exp(-tau), tau =
sum kappa_j (Y_j+1 - Y_j) over all boxes.

The march's cumulative sample counts sit at Y'_j = Y_j + E_j / step with E_j in [-below_j,
above_j], the intervals derived above (entry: [0, step x droppable samples]; and 2 u (t_j - t_0)
more on either side for the float32 step, which scales every Y_j by 1 + 2 u at most).  Sample
positions are monotone along the ray on every axis, so the Y'_j are ordered like the Y_j and so is
every point between the two: no segment has negative length on the way, and C is differentiable
along it.  For the boundary between segments j-1 and j

    dC/dY_j = T_j [ (kappa_j-1 c_j-1 - kappa_j c_j) + (kappa_j - kappa_j-1) B_j ]

with T_j the transmittance in front of the boundary (earlier boxes included) and B_j the colour
behind it per unit transmittance, B_j = sum_i>=j (T_i / T_j) c_i (1 - ...) <= 1 - (what is left
behind) <= 1 and >= 0 because the c are in [0, 1].  The bracket is linear in B: it lies between its
values D0 at B = 0 and D1 at B = 1.  Entry and exit: the same with kappa = 0 on the empty side.  A
boundary between cells of the same entry moves nothing (E taken as 0).  By the mean-value theorem
along the straight path from Y to Y',

    C_march - C_exact = sum_j dC/dY_j(xi) E_j / step,

and each term is at most T_up_j max(max(D0, D1) above_j, -min(D0, D1) below_j, 0) / step above and
T_up_j max(-min(D0, D1) above_j, max(D0, D1) below_j, 0) / step below: ONE-SIDED per boundary and
sign, as for the column.
T_up_j bounds T_j(xi) = exp(-tau'_j).  Summation by parts, with e_i = E_i / step and kappa_-1 = 0:

    tau'_j = sum_i<j kappa_i (Y'_i+1 - Y'_i) = tau_j + kappa_j-1 e_j - sum_i<j (kappa_i - kappa_i-1) e_i
           >= tau_j - [ kappa_j-1 below_j + sum_i<j ((kappa_i - kappa_i-1)^+ above_i
                                                     + (kappa_i-1 - kappa_i)^+ below_i) ] / step

the sum running over the entry (jump +kappa_first) and the cell changes before j, of this box and
of every box in front (each with its exit's term).  T_up_j = exp(-max(that bound, 0)).  This is NOT
the shorter T_j (1 - a_max)^(-s), s the largest |E| / step so far: with opacity alternating from
cell to cell and every boundary moved towards the more opaque side, the optical depth in front
drops by more than kappa_max s, so that form is no bound; the one above is, and where kappa is
constant it gives the exact kappa (below_j + entry drop) / step.
Alpha: the same argument with c = 1 needs no linearisation, tau' being monotone in each E_j: the
march's tau lies in [tau - slack_lo, tau + slack_hi], slack_lo the bracket above at the exit of
every box, slack_hi its mirror image (above and below exchanged).  For the homogeneous map this
is NO TIGHTER than alpha_lo / alpha_hi, which also use that a sample count is an integer.

Segments flagged `near` (an end within delta of a cell edge): at most l_c / step + 1 samples, each
possibly read from one of the 26 neighbours n or dropped as outside.  Replacing (a, c) of one
sample by (a_n, c_n) changes its own term by T (a c - a_n c_n) and scales all behind it, B T (a_n
- a) with B in [0, 1]: at most T_up (|a c - a_n c_n| + |a - a_n|); dropped, T_up (a c + a).  Both
are added (the safe reading), to either side; for alpha T_up (max_n |a - a_n| + a).

float32 rounding, in units of u on values <= 1 (A, C, a, c, 1 - A are all in [0, 1]); a
perturbation d of A or of a weight changes the final colour by at most d, because everything behind
is scaled by (1 - d / T) and is at most T.  Per sample and channel (AVR_ACCUMULATE, and its packed
form AVR_STEP, the same operations): 1 - A, a (1 - A), A + alpha (3, acting through the weight or
through A), c alpha and C + c alpha (2): k_1 = 5; alpha alone: the product and the sum as
check_alpha counts them, 2.  Per box crossed (blend_depthsort, once per layer in the run's fold,
the receiver's fold and the ranks' fold alike): t = 1 - front.a, back.c t, front.c + that (3) and
the same three on alpha, which act on the colour behind (3): k_2 = 6; alpha alone 3.  Once: the
clamps to [0, 1] move a value towards the exact one, which lies there, and round nothing; the
store is of a float32; the exchange and gather copy bits; the picture's byte is int(c * 256), exact
in float32 and monotone; 1 is kept for the float64 evaluation of the reference itself: k_3 = 1;
alpha alone 2, as in check_alpha (the tables here are the float32 entries themselves).
    rounding = (k_1 samples_hi + k_2 boxes_crossed + k_3) u
The stop at acc_a >= 1: what the march leaves out is at most the transmittance where it stops,
and float32 alpha can read 1 only when the exact transmittance is within alpha's rounding bound:
that bound, (2 samples_hi + 3 boxes_crossed + 2) u, is added once more to the colour.

Pixels excluded: those for which some box is hit by the ray when grown by delta but not when
shrunk by delta (hit or miss is itself uncertain).  Nothing else.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

U = 2.0 ** -24
C_POSITION = 49 + 1 + 1 + 3 + 1 + 2 + 5   # = 62; the count is in the module docstring
MESH_EPSILON = 1e-4      # of the box diagonal (VolumePainter.cpp:692)


@dataclass
class Conventions:
    """The reading of the camera stated in the module docstring.  Other values exist only so that
    the tests can show the brackets tell a different reading apart."""
    pixel_centre: float = 0.5
    row0_at_bottom: bool = True
    fov_is_full_angle: bool = True
    aspect_on_x: bool = True


@dataclass
class Reading:
    """The reading of the coloured picture stated in the module docstring (emission-absorption).
    Other values exist only so that the tests can show the colour brackets tell them apart."""
    boxes_front_to_back: bool = True
    segments_front_to_back: bool = True
    colour_times_opacity: bool = True     # False: the table's colour taken as premultiplied
    entry_offset: int = 0                 # table[k + entry_offset] for a cell of entry k
    boxes_shadow: bool = True             # False: layers summed without what is in front
    swap_red_blue: bool = False


@dataclass
class Box:
    min_corner: Sequence[float]
    max_corner: Sequence[float]
    cells: np.ndarray                  # float64 [nz, ny, nx], may be a strided view
    index: Optional[np.ndarray] = None  # integer colour-table entry per cell, for MIP
    level: int = 0

    @property
    def lo(self):
        return np.asarray(self.min_corner, np.float64)

    @property
    def hi(self):
        return np.asarray(self.max_corner, np.float64)

    @property
    def dims(self):
        nz, ny, nx = self.cells.shape
        return np.array([nx, ny, nz])

    @property
    def spacing(self):
        return (self.hi - self.lo) / self.dims

    @property
    def step(self):
        return float(self.spacing.min()) * 0.5

    @property
    def mesh_epsilon(self):
        return MESH_EPSILON * float(np.linalg.norm(self.hi - self.lo))


def camera_frame(camera):
    eye = np.asarray(camera.eye, np.float64)
    f = np.asarray(camera.look_at, np.float64) - eye
    f = f / np.linalg.norm(f)
    r = np.cross(f, np.asarray(camera.up, np.float64))
    r = r / np.linalg.norm(r)
    return eye, f, r, np.cross(r, f)


def rays(camera, width: int, height: int, conventions: Conventions = Conventions()) -> np.ndarray:
    """Unit directions [height, width, 3]; row 0 first."""
    _, f, r, u = camera_frame(camera)
    c = conventions
    half = np.radians(np.float64(camera.fov_y_degrees)) * (0.5 if c.fov_is_full_angle else 1.0)
    tan_half = np.tan(half)
    aspect = width / height
    px = (2.0 * (np.arange(width) + c.pixel_centre) / width - 1.0) * tan_half
    py = (2.0 * (np.arange(height) + c.pixel_centre) / height - 1.0) * tan_half
    if c.aspect_on_x:
        px = px * aspect
    else:
        py = py * aspect
    if not c.row0_at_bottom:
        py = -py
    D = f[None, None, :] + px[None, :, None] * r[None, None, :] + py[:, None, None] * u[None, None, :]
    return D / np.linalg.norm(D, axis=-1, keepdims=True)


def slab(origin, d, lo, hi):
    """Entry and exit parameter of rays origin + t d [P, 3] through the box [lo, hi] (lo, hi: [3]
    or [P, 3]); entry > exit where the ray misses."""
    lo = np.broadcast_to(lo, d.shape)
    hi = np.broadcast_to(hi, d.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (lo - origin) / d
        t2 = (hi - origin) / d
    near, far = np.minimum(t1, t2), np.maximum(t1, t2)
    parallel = d == 0.0
    inside = (origin >= lo) & (origin <= hi)
    near = np.where(parallel, np.where(inside, -np.inf, np.inf), near)
    far = np.where(parallel, np.where(inside, np.inf, -np.inf), far)
    return near.max(axis=1), far.min(axis=1)


@dataclass
class Chords:
    rays: np.ndarray       # indices (into the P rays) of those that cross the box
    t_in: np.ndarray       # [R] entry parameter, NOT clamped at the eye (negative: eye inside)
    t_out: np.ndarray      # [R]
    t: np.ndarray          # [R, S + 1] sorted segment boundaries within [max(t_in, 0), t_out]
    axis: np.ndarray       # [R, S + 1] axis of the plane crossed at each boundary
    cell: np.ndarray       # [R, S, 3] (i, j, k) of each segment
    length: np.ndarray     # [R, S] l_c (0 for the empty segments the merge leaves)
    delta: np.ndarray      # [R] position uncertainty in this box
    tangential: np.ndarray  # [P] hit or miss uncertain


def position_delta(origin, t_out, chord, step):
    k = np.ceil(chord / step) + 1.0
    return (C_POSITION + k) * U * (np.abs(origin).max() + t_out)


def chords(origin, d, box: Box) -> Chords:
    """Exact traversal of `box` by the rays origin + t d, d: [P, 3] unit vectors."""
    origin = np.asarray(origin, np.float64)
    lo, hi, dims, h = box.lo, box.hi, box.dims, box.spacing
    t_in, t_out = slab(origin, d, lo, hi)
    start = np.maximum(t_in, 0.0)
    hit = t_out > start
    # hit or miss uncertain: the box grown and shrunk by delta disagree
    far = np.where(np.isfinite(t_out), np.maximum(t_out, 0.0), 0.0) + np.linalg.norm(hi - lo)
    dl = position_delta(origin, far, np.linalg.norm(hi - lo), box.step)[:, None]
    g_in, g_out = slab(origin, d, lo - dl, hi + dl)
    s_in, s_out = slab(origin, d, lo + dl, hi - dl)
    tangential = (g_out > np.maximum(g_in, 0.0)) != (s_out > np.maximum(s_in, 0.0))

    idx = np.nonzero(hit)[0]
    d, t_in, t_out, start = d[idx], t_in[idx], t_out[idx], start[idx]
    planes, axes = [], []
    for a in range(3):
        p = lo[a] + (hi[a] - lo[a]) * (np.arange(dims[a] + 1) / dims[a])
        p[-1] = hi[a]
        with np.errstate(divide="ignore", invalid="ignore"):
            ta = (p[None, :] - origin[a]) / d[:, a:a + 1]
        planes.append(np.where(np.isfinite(ta), ta, np.inf))
        axes.append(np.full(dims[a] + 1, a))
    t = np.concatenate(planes, axis=1)
    axis = np.broadcast_to(np.concatenate(axes)[None, :], t.shape)
    order = np.argsort(t, axis=1, kind="stable")
    t = np.take_along_axis(t, order, axis=1)
    axis = np.take_along_axis(axis, order, axis=1)
    t = np.clip(t, start[:, None], t_out[:, None])
    length = np.diff(t, axis=1)
    mid = 0.5 * (t[:, 1:] + t[:, :-1])
    pos = origin[None, None, :] + mid[:, :, None] * d[:, None, :]
    cell = np.floor((pos - lo) / h).astype(np.int64)
    cell = np.clip(cell, 0, dims - 1)
    delta = position_delta(origin, t_out, t_out - start, box.step)
    return Chords(idx, t_in, t_out, t, axis, cell, length, delta, tangential)


def _dilate(a, reduce):
    """reduce (np.maximum / np.minimum) over the 3x3x3 neighbourhood, edges clamped."""
    out = a
    for ax in range(3):
        n = out.shape[ax]
        up = np.take(out, np.minimum(np.arange(n) + 1, n - 1), axis=ax)
        down = np.take(out, np.maximum(np.arange(n) - 1, 0), axis=ax)
        out = reduce(out, reduce(up, down))
    return out


# float32 roundings, in units of U on values <= 1 (module docstring, "float32 rounding"): per
# sample, per box crossed, once per pixel; for a colour channel and for alpha
K_COLOUR = (5, 6, 1)
K_ALPHA = (2, 3, 2)


@dataclass
class ColourTerms:
    """Per ray that crosses the box (Chords.rays).  `under`, `over`, `alpha_near` are per unit of
    the transmittance in front of the box; the tau_* widen the box's optical depth tau."""
    entry: np.ndarray        # [R] where the ray enters the box (0: the eye is inside)
    layer: np.ndarray        # [R, 3] L_b
    under: np.ndarray        # [R, 3]
    over: np.ndarray         # [R, 3]
    tau: np.ndarray          # [R] -log(1 - A_b)
    tau_under: np.ndarray    # [R] the march's optical depth lies in [tau - under, tau + over]
    tau_over: np.ndarray
    alpha_near: np.ndarray   # [R] the near-an-edge term of alpha
    samples_hi: np.ndarray   # [R]


def _neighbour_spread(q):
    """q: [nz, ny, nx, 4], a cell's (r, g, b, a).  What one sample of a cell may be wrong by per
    unit transmittance when it is read from one of the 26 neighbours (edges clamped) or dropped:
    max_n (|a c - a_n c_n| + |a - a_n|) + (a c + a)  [nz, ny, nx, 3],  and with c = 1 for alpha
    max_n |a - a_n| + a  [nz, ny, nx]."""
    a = q[..., 3]
    ac = q[..., :3] * a[..., None]
    worst_c, worst_a = np.zeros(ac.shape), np.zeros(a.shape)
    at = [np.arange(n) for n in a.shape]
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if not (dz or dy or dx):
                    continue
                sel = np.ix_(*[np.clip(at[ax] + s, 0, a.shape[ax] - 1)
                               for ax, s in enumerate((dz, dy, dx))])
                da = np.abs(a - a[sel])
                worst_a = np.maximum(worst_a, da)
                worst_c = np.maximum(worst_c, np.abs(ac - ac[sel]) + da[..., None])
    return worst_c + ac + a[..., None], worst_a + a


def _colour_terms(box, ch, table, step, reading, real, near, first, last, below, above,
                  entry_above, samples_hi) -> ColourTerms:
    """The box's layer and its margins (module docstring, "Colour").  real, near, first, last,
    below, above, entry_above: box_terms' own."""
    assert box.index is not None and table.shape == (256, 4)
    # opaque entries (a = 1, kappa infinite) and colours outside [0, 1] are out of scope
    assert (table[:, :3] >= 0.0).all() and (table[:, :3] <= 1.0).all()
    assert (table[:, 3] >= 0.0).all() and (table[:, 3] < 1.0).all()
    R, S = ch.length.shape
    rows = np.arange(R)
    i, j, k = ch.cell[..., 0], ch.cell[..., 1], ch.cell[..., 2]
    assert np.isfinite(box.cells[k, j, i][real]).all()     # cells are finite here
    entries = np.clip(box.index.astype(np.int64) + reading.entry_offset, 0, 255)
    m = entries[k, j, i]
    a, c = table[m, 3], table[m, :3]                        # [R, S], [R, S, 3]
    kap = -np.log1p(-a)
    dY = ch.length / step
    tau_seg = kap * dY
    seg_alpha = -np.expm1(-tau_seg)

    # ---- the exact layer
    if reading.segments_front_to_back:
        in_front = np.cumsum(tau_seg, axis=1) - tau_seg
    else:
        in_front = tau_seg.sum(axis=1, keepdims=True) - np.cumsum(tau_seg, axis=1)
    if reading.colour_times_opacity:
        weight = seg_alpha
    else:       # C += c (1 - A) per sample: the geometric sum over the segment's samples
        weight = np.where(a > 0.0, seg_alpha / np.where(a > 0.0, a, 1.0), dY)
    layer = ((np.exp(-in_front) * weight)[..., None] * c).sum(axis=1)
    if reading.swap_red_blue:
        layer = layer[:, ::-1]
    tau = tau_seg.sum(axis=1)

    # ---- boundaries 0 .. S: (kappa, c) in front of (f) and behind (b) each; the last real
    # segment's values carried over the empty ones, so that jumps are between real cells
    carry = np.maximum.accumulate(np.where(real, np.arange(S)[None, :], 0), axis=1)
    kc = np.take_along_axis(kap, carry, axis=1)
    cc = np.take_along_axis(c, carry[..., None], axis=1)
    inner = np.arange(1, S)[None, :] > first[:, None]
    kf, kb = np.zeros((R, S + 1)), np.zeros((R, S + 1))
    cf, cb = np.zeros((R, S + 1, 3)), np.zeros((R, S + 1, 3))
    kf[:, 1:S], kb[:, 1:S] = np.where(inner, kc[:, :-1], 0.0), np.where(inner, kc[:, 1:], 0.0)
    cf[:, 1:S] = np.where(inner[..., None], cc[:, :-1], 0.0)
    cb[:, 1:S] = np.where(inner[..., None], cc[:, 1:], 0.0)
    kb[rows, first], cb[rows, first] = kap[rows, first], c[rows, first]          # the entry
    kf[rows, last + 1], cf[rows, last + 1] = kap[rows, last], c[rows, last]      # the exit
    kb[rows, last + 1], cb[rows, last + 1] = 0.0, 0.0
    D0 = kf[..., None] * cf - kb[..., None] * cb            # dC/dY_j / T_j at B = 0 ...
    D1 = D0 + (kb - kf)[..., None]                          # ... and at B = 1
    dmax, dmin = np.maximum(D0, D1), np.minimum(D0, D1)

    # ---- E_j in [-e_lo, e_hi] where moving the boundary changes anything; the float32 step
    # (2 u relative on every Y_j) is a shift of 2 u (t_j - t_0) more
    moves = (kf != kb) | (D0 != 0.0).any(axis=-1)
    grow = 2.0 * U * (ch.t - ch.t[:, :1])
    e_lo = np.where(moves, below + grow, 0.0)
    e_hi = np.where(moves, above + grow, 0.0)
    e_lo[rows, first], e_hi[rows, first] = 0.0, entry_above
    assert np.isfinite(e_lo).all() and np.isfinite(e_hi).all()

    # ---- the optical depth in front of boundary j, from below and from above (summation by parts)
    tau_front = np.concatenate([np.zeros((R, 1)), np.cumsum(tau_seg, axis=1)], axis=1)
    up, down = np.maximum(kb - kf, 0.0), np.maximum(kf - kb, 0.0)
    less, more = up * e_hi + down * e_lo, up * e_lo + down * e_hi
    slack_lo = (kf * e_lo + np.cumsum(less, axis=1) - less) / step
    slack_hi = (kf * e_hi + np.cumsum(more, axis=1) - more) / step
    T_up = np.exp(-np.maximum(tau_front - slack_lo, 0.0))

    over = (T_up[..., None] * np.maximum(np.maximum(dmax * e_hi[..., None], -dmin * e_lo[..., None]),
                                         0.0)).sum(axis=1) / step
    under = (T_up[..., None] * np.maximum(np.maximum(-dmin * e_hi[..., None], dmax * e_lo[..., None]),
                                          0.0)).sum(axis=1) / step
    spread_c, spread_a = _neighbour_spread(table[entries])
    wrong = np.where(near, dY + 1.0, 0.0) * T_up[:, :-1]
    lateral = (wrong[..., None] * spread_c[k, j, i]).sum(axis=1)
    return ColourTerms(ch.t[:, 0], layer, under + lateral, over + lateral, tau,
                       slack_lo[rows, last + 1], slack_hi[rows, last + 1],
                       (wrong * spread_a[k, j, i]).sum(axis=1), samples_hi)


@dataclass
class BoxTerms:
    """Per ray that crosses the box (Chords.rays): exact integrals and derived margins."""
    ch: Chords
    length: np.ndarray
    length_margin: tuple       # (under, over): got lies in [exact - under, exact + over]
    column: np.ndarray
    column_margin: tuple
    mip_lo: Optional[np.ndarray]
    mip_hi: Optional[np.ndarray]
    depth: np.ndarray
    depth_margin: np.ndarray
    lateral: np.ndarray = None   # [R] bool: some segment carries the near-an-edge term
    colour: Optional["ColourTerms"] = None   # with a colour table only


def box_terms(camera, d, box: Box, step: Optional[float] = None, table=None,
              reading: Reading = Reading()) -> BoxTerms:
    """d: [P, 3].  `step` overrides the box's own step (tests of the brackets' teeth only).
    table: float64 [256, 4] (r, g, b, opacity of one sample) of this box's level; with it and
    box.index the box's colour layer and its margins are filled in (BoxTerms.colour)."""
    origin, f, _, _ = camera_frame(camera)
    ch = chords(origin, d, box)
    dr = d[ch.rays]
    step = box.step if step is None else step
    eps = box.mesh_epsilon
    lo, h = box.lo, box.spacing
    i, j, k = ch.cell[..., 0], ch.cell[..., 1], ch.cell[..., 2]
    v = box.cells[k, j, i]
    finite = np.isfinite(v)
    v = np.where(finite, v, 0.0)
    w = finite.astype(np.float64)
    real = ch.length > 0.0
    delta = ch.delta[:, None]
    abs_d = np.abs(dr)
    with np.errstate(divide="ignore"):
        tau = delta / np.take_along_axis(abs_d, ch.axis, axis=1)          # [R, S + 1]

    # near an edge: an end of the segment within delta of a cell face other than the one crossed
    near = np.zeros(ch.length.shape, bool)
    for end in (0, 1):
        te = ch.t[:, end:ch.t.shape[1] - 1 + end]
        ax = ch.axis[:, end:ch.axis.shape[1] - 1 + end]
        p = origin[None, None, :] + te[:, :, None] * dr[:, None, :]
        rel = (p - lo) / h - ch.cell                                      # in [0, 1] inside the cell
        dist = np.minimum(rel, 1.0 - rel) * h
        for a in range(3):
            near |= (ax != a) & (dist[..., a] <= delta)
    near &= real

    # E_j in [-below_j, above_j] at every boundary; the first and last boundaries with l > 0 are
    # the entry and the exit
    below = eps + delta + tau
    above = max(step - eps, 0.0) + delta + tau
    R, S = ch.length.shape
    first = np.argmax(real, axis=1)
    last = S - 1 - np.argmax(real[:, ::-1], axis=1)
    rows = np.arange(R)
    reach = tau[rows, first] + ch.delta - eps       # how far past the entry a sample may be dropped
    entry_above = np.where(reach < 0.0, 0.0, step * (np.floor(np.maximum(reach, 0.0) / step) + 1.0))
    exit_below, exit_above = below[rows, last + 1], above[rows, last + 1]

    def margin(q, spread):
        """(under, over): step * sum over samples of q lies in [exact - under, exact + over]."""
        # carry the last real segment's q over the empty ones, so that jumps are between real cells
        pos_idx = np.where(real, np.arange(S)[None, :], 0)
        carried = np.take_along_axis(q, np.maximum.accumulate(pos_idx, axis=1), axis=1)
        jump = np.diff(carried, axis=1)                                   # at boundaries 1 .. S - 1
        jump = np.where(np.arange(1, S)[None, :] > first[:, None], jump, 0.0)
        assert not (np.isinf(tau[:, 1:S]) & (jump != 0.0)).any()
        lo_j = np.where(jump != 0.0, below[:, 1:S], 0.0)
        hi_j = np.where(jump != 0.0, above[:, 1:S], 0.0)
        up, down = np.maximum(jump, 0.0), np.maximum(-jump, 0.0)
        # error = - sum_j jump_j E_j, with jump = +q_first at the entry and -q_last at the exit
        q0, q1 = q[rows, first], q[rows, last]
        over = (up * lo_j + down * hi_j).sum(axis=1) + np.maximum(-q0, 0.0) * entry_above \
            + np.maximum(q1, 0.0) * exit_above + np.maximum(-q1, 0.0) * exit_below
        under = (up * hi_j + down * lo_j).sum(axis=1) + np.maximum(q0, 0.0) * entry_above \
            + np.maximum(q1, 0.0) * exit_below + np.maximum(-q1, 0.0) * exit_above
        lateral = (near * (ch.length + step) * spread).sum(axis=1)
        return under + lateral, over + lateral

    length = (w * ch.length).sum(axis=1)
    column = (v * ch.length).sum(axis=1)
    vmax, vmin = _dilate(np.where(np.isfinite(box.cells), box.cells, 0.0), np.maximum), \
        _dilate(np.where(np.isfinite(box.cells), box.cells, 0.0), np.minimum)
    spread_v = np.maximum(np.maximum(vmax[k, j, i] - v, v - vmin[k, j, i]), np.abs(v))
    length_margin = tuple(m + 2.0 * U * length for m in margin(w, np.ones_like(w)))
    column_margin = tuple(m + 2.0 * U * np.abs(v * ch.length).sum(axis=1)
                          for m in margin(v, spread_v))

    mip_lo = mip_hi = None
    if box.index is not None:
        m = box.index[k, j, i].astype(np.int64)
        s0 = np.maximum(ch.t_in, 0.0) + eps + ch.delta
        a = np.maximum(ch.t[:, :-1] + tau[:, :-1], s0[:, None])
        b = ch.t[:, 1:] - tau[:, 1:]
        certain = real & ~near & (b - a > step * (1.0 + 2.0 * U))
        mip_lo = np.where(certain, m, -1).max(axis=1)
        wide = _dilate(box.index.astype(np.int64), np.maximum)[k, j, i]
        mip_hi = np.where(real, np.where(near, wide, m), -1).max(axis=1)

    # depth of the layer: (entry point - eye) . forward, the entry NOT clamped at the eye (:914-919)
    cos = dr @ f
    depth = ch.t_in * cos
    entry_axis = np.argmax(np.where(dr != 0.0, np.where(dr > 0, lo - origin, box.hi - origin) /
                                    np.where(dr != 0.0, dr, 1.0), -np.inf), axis=1)
    tau_in = ch.delta / abs_d[rows, entry_axis]
    # entry point: 3 components x (position delta + subtract + multiply) + 2 adds of the dot product
    depth_margin = tau_in * np.abs(cos) + 3.0 * ch.delta + \
        8.0 * U * (np.abs(origin).max() + np.abs(ch.t_in))
    colour = None
    if table is not None:
        colour = _colour_terms(box, ch, np.asarray(table, np.float64), step, reading, real, near,
                               first, last, below, above, entry_above,
                               np.floor((length + length_margin[1]) / step))
    return BoxTerms(ch, length, length_margin, column, column_margin, mip_lo, mip_hi, depth,
                    depth_margin, near.any(axis=1), colour)


@dataclass
class Expected:
    """Images [height, width], row 0 at the bottom."""
    hit: np.ndarray            # the ray crosses some box
    excluded: np.ndarray       # hit or miss of some box uncertain
    length: np.ndarray
    length_under: np.ndarray   # got lies in [length - length_under, length + length_over]
    length_over: np.ndarray
    column: np.ndarray
    column_under: np.ndarray
    column_over: np.ndarray
    mip_lo: np.ndarray
    mip_hi: np.ndarray
    boxes_crossed: np.ndarray
    lateral: np.ndarray = None   # pixels whose brackets carry a near-an-edge term in some box
    alpha_lo: Optional[np.ndarray] = None
    alpha_hi: Optional[np.ndarray] = None
    samples_hi: Optional[np.ndarray] = None
    # the same with n_b in [floor(l_b / step_b), ceil(l_b / step_b)], l_b the exact chord: what
    # a medium of the table's opacity per reference step must fall inside whatever the phase
    physical_lo: Optional[np.ndarray] = None
    physical_hi: Optional[np.ndarray] = None
    # with colour tables: the premultiplied colour [height, width, 3] and the alpha of the
    # emission-absorption picture, got in [x - x_under, x + x_over] per channel
    colour: Optional[np.ndarray] = None
    colour_under: Optional[np.ndarray] = None
    colour_over: Optional[np.ndarray] = None
    alpha: Optional[np.ndarray] = None
    alpha_under: Optional[np.ndarray] = None
    alpha_over: Optional[np.ndarray] = None

    def outside(self, what: str, got) -> np.ndarray:
        """Where `got` leaves the bracket of "length", "column", "alpha" or "colour" (there: in
        any channel)."""
        exact = getattr(self, what)
        bad = (got < exact - getattr(self, what + "_under")) | \
            (got > exact + getattr(self, what + "_over"))
        return bad.any(axis=-1) if bad.ndim == 3 else bad

    def lateral_share(self) -> float:
        """Share of the hitting pixels whose brackets are widened by the near-an-edge term."""
        return float((self.lateral & self.hit).sum()) / max(int(self.hit.sum()), 1)

    def excluded_share(self) -> float:
        return float((self.excluded & self.hit).sum()) / max(int(self.hit.sum()), 1)


def expected(camera, width: int, height: int, boxes: Sequence[Box],
             steps: Optional[Sequence[float]] = None,
             sample_alpha: Optional[Sequence[float]] = None,
             conventions: Conventions = Conventions(),
             tables: Optional[Sequence[np.ndarray]] = None,
             reading: Reading = Reading()) -> Expected:
    """Exact images over disjoint boxes, and the brackets a stepping march must stay inside.
    sample_alpha[b]: the opacity one sample of box b adds in a homogeneous medium.
    tables[b]: the colour table [256, 4] of box b's level (boxes then carry .index): fills
    colour, alpha and their margins.  `reading` other than the default changes the exact colour
    only (the margins are those of the default reading)."""
    d = rays(camera, width, height, conventions).reshape(-1, 3)
    P = d.shape[0]
    z = lambda: np.zeros(P)  # noqa: E731
    out = Expected(np.zeros(P, bool), np.zeros(P, bool), z(), z(), z(), z(), z(), z(),
                   np.full(P, -1, np.int64), np.full(P, -1, np.int64), np.zeros(P, np.int64))
    log_t_lo, log_t_hi, n_hi_total, log_p_lo, log_p_hi = z(), z(), z(), z(), z()
    lateral = np.zeros(P, bool)
    if tables is not None:
        # per ray and box, to be put in the order of the entries along the ray
        col = {name: np.zeros((P, len(boxes)) + tail) for name, tail in (
            ("layer", (3,)), ("under", (3,)), ("over", (3,)), ("tau", ()), ("tau_under", ()),
            ("tau_over", ()), ("alpha_near", ()), ("samples_hi", ()))}
        entry = np.full((P, len(boxes)), np.inf)
    for b, box in enumerate(boxes):
        step = box.step if steps is None else steps[b]
        bt = box_terms(camera, d, box, step, None if tables is None else tables[b], reading)
        r = bt.ch.rays
        out.excluded |= bt.ch.tangential
        out.hit[r] = True
        out.boxes_crossed[r] += 1
        lateral[r] |= bt.lateral
        out.length[r] += bt.length
        out.length_under[r] += bt.length_margin[0]
        out.length_over[r] += bt.length_margin[1]
        out.column[r] += bt.column
        out.column_under[r] += bt.column_margin[0]
        out.column_over[r] += bt.column_margin[1]
        if bt.mip_lo is not None:
            out.mip_lo[r] = np.maximum(out.mip_lo[r], bt.mip_lo)
            out.mip_hi[r] = np.maximum(out.mip_hi[r], bt.mip_hi)
        if sample_alpha is not None:
            n_lo = np.maximum(np.ceil((bt.length - bt.length_margin[0]) / step), 0.0)
            n_hi = np.floor((bt.length + bt.length_margin[1]) / step)
            keep = np.log1p(-float(sample_alpha[b]))
            log_t_hi[r] += n_lo * keep
            log_t_lo[r] += n_hi * keep
            n_hi_total[r] += n_hi
            log_p_hi[r] += np.floor(bt.length / step) * keep
            log_p_lo[r] += np.ceil(bt.length / step) * keep
        if tables is not None:
            entry[r, b] = bt.colour.entry
            for name, values in col.items():
                values[r, b] = getattr(bt.colour, name)
    shape = (height, width)
    for name in ("hit", "excluded", "length", "length_under", "length_over", "column", "column_under",
                 "column_over", "mip_lo",
                 "mip_hi", "boxes_crossed"):
        setattr(out, name, getattr(out, name).reshape(shape))
    out.lateral = lateral.reshape(shape)
    if sample_alpha is not None:
        out.alpha_lo = (-np.expm1(log_t_hi)).reshape(shape)
        out.alpha_hi = (-np.expm1(log_t_lo)).reshape(shape)
        out.samples_hi = n_hi_total.reshape(shape)
        out.physical_lo = (-np.expm1(log_p_hi)).reshape(shape)
        out.physical_hi = (-np.expm1(log_p_lo)).reshape(shape)
    if tables is not None:
        _compose_colour(out, entry, col, reading, shape)
    return out


def _compose_colour(out: Expected, entry, col, reading: Reading, shape) -> None:
    """The pixel from its boxes' layers in the order of their entries along the ray (missed
    boxes, entry = inf and nothing in them, come last), and the margins summed with the bound on
    the transmittance in front of each box (module docstring, "Colour")."""
    order = np.argsort(entry if reading.boxes_front_to_back else -entry, axis=1, kind="stable")
    for name, values in col.items():
        index = order if values.ndim == 2 else order[..., None]
        col[name] = np.take_along_axis(values, index, axis=1)
    tau = col["tau"]
    tau_front = np.cumsum(tau, axis=1) - tau
    slack_front = np.cumsum(col["tau_under"], axis=1) - col["tau_under"]
    t_up = np.exp(-np.maximum(tau_front - slack_front, 0.0))
    t_front = np.exp(-tau_front) if reading.boxes_shadow else np.ones_like(tau_front)
    samples = col["samples_hi"].sum(axis=1)
    crossed = out.boxes_crossed.reshape(-1)
    rounding = {what: (k[0] * samples + k[1] * crossed + k[2]) * U
                for what, k in (("colour", K_COLOUR), ("alpha", K_ALPHA))}
    rounding["colour"] = rounding["colour"] + rounding["alpha"]     # the stop at alpha >= 1
    out.colour = (t_front[..., None] * col["layer"]).sum(axis=1).reshape(shape + (3,))
    for side in ("under", "over"):
        margin = (t_up[..., None] * col[side]).sum(axis=1) + rounding["colour"][:, None]
        setattr(out, "colour_" + side, margin.reshape(shape + (3,)))
    total = tau.sum(axis=1)
    alpha = -np.expm1(-total)
    near = (t_up * col["alpha_near"]).sum(axis=1) + rounding["alpha"]
    lowest = -np.expm1(-np.maximum(total - col["tau_under"].sum(axis=1), 0.0))
    highest = -np.expm1(-(total + col["tau_over"].sum(axis=1)))
    out.alpha = alpha.reshape(shape)
    out.alpha_under = (alpha - lowest + near).reshape(shape)
    out.alpha_over = (highest - alpha + near).reshape(shape)
    if out.samples_hi is None:
        out.samples_hi = samples.reshape(shape)


# ---- AMR hierarchies given as levels with overlap ----------------------------------------------

def finest_value_grid(levels: Sequence[dict], ref_ratio: Sequence[int]) -> np.ndarray:
    """The finest-level value at every point of the domain, as a dense array [nz, ny, nx] at the
    finest level's resolution: each level, coarse to fine, overwrites what lies under it.
    levels[l] = {"domain": (lo, hi), "boxes": [(lo, hi)], "data": [array [nz, ny, nx]]}, index
    boxes inclusive and cell-centred (lo of level 0's domain must be 0)."""
    (dlo, dhi) = levels[0]["domain"]
    assert tuple(dlo) == (0, 0, 0)
    grid = np.full(tuple(dhi[a] + 1 for a in (2, 1, 0)), np.nan)
    for level, lev in enumerate(levels):
        if level > 0:
            r = int(ref_ratio[level - 1])
            for ax in range(3):
                grid = np.repeat(grid, r, axis=ax)
        for (lo, hi), data in zip(lev["boxes"], lev["data"]):
            grid[lo[2]:hi[2] + 1, lo[1]:hi[1] + 1, lo[0]:hi[0] + 1] = data
    return grid


def coverage_count(level_index_boxes: Sequence[Sequence], ref_ratio: Sequence[int],
                   domain_hi) -> np.ndarray:
    """How many of the given per-level index boxes [(lo, hi)] cover each finest-level cell."""
    n_levels = len(level_index_boxes)
    scale = [1] * n_levels
    for level in range(n_levels - 2, -1, -1):
        scale[level] = scale[level + 1] * int(ref_ratio[level])
    count = np.zeros(tuple((domain_hi[a] + 1) * scale[0] for a in (2, 1, 0)), np.int64)
    for level, boxes in enumerate(level_index_boxes):
        s = scale[level]
        for lo, hi in boxes:
            count[lo[2] * s:(hi[2] + 1) * s, lo[1] * s:(hi[1] + 1) * s,
                  lo[0] * s:(hi[0] + 1) * s] += 1
    return count
