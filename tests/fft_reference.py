"""The definitions of DESIGN.md 7, "Power spectrum", in numpy: the twiddle table, the radix-2
transform of one line with its loops in the stated order, the same butterflies on many lines at
once, the 3-D transform (x, then y, then z) and the shell sums.  numpy's elementwise float64
arithmetic rounds every product and sum on its own, which is what the kernels do.  Apart from that
restatement, and sharing nothing with it: the transform and its inverse by their definition in
long double (exact_fft3d, exact_ifft3d) and the closed forms of one cell and of one mode
(delta_spectrum, plane_wave), what the restatement and the kernels are held to."""
import math

import numpy as np


def twiddles(n):
    """W[m] = (cos t, sin t), t = -(2.0 pi m) / n in that order, for m in [0, n / 2): [n / 2, 2]."""
    table = np.zeros((n // 2, 2), dtype=np.float64)
    for m in range(n // 2):
        theta = -(2.0 * math.pi * m) / n
        table[m, 0] = math.cos(theta)
        table[m, 1] = math.sin(theta)
    return table


def bit_reverse(index, p):
    out = 0
    for bit in range(p):
        out |= ((index >> bit) & 1) << (p - 1 - bit)
    return out


def fft_line_loops(re, im):
    """One line, every loop written out: (re, im) float64 [n] -> the transform, new arrays."""
    n = len(re)
    p = n.bit_length() - 1
    assert 1 << p == n
    w = twiddles(n)
    vr = np.array([re[bit_reverse(i, p)] for i in range(n)], dtype=np.float64)
    vi = np.array([im[bit_reverse(i, p)] for i in range(n)], dtype=np.float64)
    for s in range(1, p + 1):
        half, step = 1 << (s - 1), n >> s
        for block in range(0, n, 2 * half):
            for j in range(half):
                ar, ai = vr[block + j], vi[block + j]
                br, bi = vr[block + j + half], vi[block + j + half]
                wr, wi = w[j * step]
                tr = np.float64(wr * br) - np.float64(wi * bi)
                ti = np.float64(wr * bi) + np.float64(wi * br)
                vr[block + j], vi[block + j] = ar + tr, ai + ti
                vr[block + j + half], vi[block + j + half] = ar - tr, ai - ti
    return vr, vi


def fft_lines(re, im):
    """The same butterflies on the last axis of (re, im) float64 [..., n], all lines at once."""
    n = re.shape[-1]
    p = n.bit_length() - 1
    assert 1 << p == n
    w = twiddles(n)
    order = np.array([bit_reverse(i, p) for i in range(n)], dtype=np.int64)
    vr, vi = np.array(re[..., order]), np.array(im[..., order])
    lead = vr.shape[:-1]
    for s in range(1, p + 1):
        half, step = 1 << (s - 1), n >> s
        wr, wi = w[np.arange(half) * step, 0], w[np.arange(half) * step, 1]
        vr = vr.reshape(lead + (n // (2 * half), 2, half))
        vi = vi.reshape(lead + (n // (2 * half), 2, half))
        ar, ai = vr[..., 0, :], vi[..., 0, :]
        br, bi = vr[..., 1, :], vi[..., 1, :]
        tr = wr * br - wi * bi
        ti = wr * bi + wi * br
        vr = np.stack([ar + tr, ar - tr], axis=-2).reshape(lead + (n,))
        vi = np.stack([ai + ti, ai - ti], axis=-2).reshape(lead + (n,))
    return vr, vi


def fft3d(values):
    """Real float64 [nz, ny, nx] -> float64 [nz, ny, nx, 2]: along x, then y, then z."""
    re = np.array(values, dtype=np.float64)
    im = np.zeros_like(re)
    for axis in (2, 1, 0):
        re, im = np.moveaxis(re, axis, -1), np.moveaxis(im, axis, -1)
        re, im = fft_lines(re, im)
        re, im = np.moveaxis(re, -1, axis), np.moveaxis(im, -1, axis)
    return np.ascontiguousarray(np.stack([re, im], axis=-1))


# ---- the transform by its definition, in long double -------------------------------------------
# None of what follows shares code or algorithm with the radix-2 restatement above: a dense matrix
# per axis, its phases from exact integer indices, everything in numpy.longdouble.

def require_long_double():
    """The long-double helpers are a reference only where long double is wider than float64."""
    eps = float(np.finfo(np.longdouble).eps)
    assert eps <= 2.0 ** -63, (
        f"numpy.longdouble has eps = {eps:g} here, not the 2^-63 or less of an extended format: "
        "the long-double reference would be no more precise than what it checks")


def long_pi():
    return np.longdouble(4) * np.arctan(np.longdouble(1))


def unit_roots(n):
    """(cos t, sin t) of t = -(2 pi m) / n for m in [0, n), long double [n] each."""
    require_long_double()
    m = np.arange(n, dtype=np.int64).astype(np.longdouble)
    theta = -(2 * long_pi() * m) / np.longdouble(n)
    return np.cos(theta), np.sin(theta)


_DFT = {}


def dft_matrix(n):
    """(C, S) long double [n, n]: exp(-2 pi i k j / n) = C[k, j] + i S[k, j], the phase index
    (k j) mod n as an exact integer.  Made once per n; read-only."""
    if n not in _DFT:
        c, s = unit_roots(n)
        k = np.arange(n, dtype=np.int64)
        index = (k[:, None] * k[None, :]) % n
        big_c, big_s = c[index], s[index]
        big_c.setflags(write=False)
        big_s.setflags(write=False)
        _DFT[n] = (big_c, big_s)
    return _DFT[n]


def _dft_axes(re, im, sign):
    """The separable DFT of (re, im) long double [nz, ny, nx] over its three axes by matrix
    products; sign = 1: exp(-i ...), sign = -1: exp(+i ...).  Unnormalised."""
    for axis in range(3):
        n = re.shape[axis]
        if n == 1:
            continue
        c, s = dft_matrix(n)                            # symmetric
        re, im = np.moveaxis(re, axis, -1), np.moveaxis(im, axis, -1)
        a, b = re @ c, sign * (re @ s)
        if im.any():                                    # not on a real grid's first axis
            a, b = a - sign * (im @ s), b + im @ c
        re, im = np.moveaxis(a, -1, axis), np.moveaxis(b, -1, axis)
    return np.ascontiguousarray(re), np.ascontiguousarray(im)


def exact_fft3d(values):
    """Real [nz, ny, nx] -> (re, im) long double [nz, ny, nx]: F[kz, ky, kx] = sum over (z, y, x)
    of v[z, y, x] exp(-2 pi i (kx x / nx + ky y / ny + kz z / nz)), the forward, unnormalised
    transform by its definition."""
    require_long_double()
    re = np.asarray(values, dtype=np.float64).astype(np.longdouble)
    return _dft_axes(re, np.zeros_like(re), 1)


def exact_ifft3d(re, im):
    """(re, im) [nz, ny, nx] -> (re, im) long double: the inverse with exp(+...) and 1 / Ntot."""
    require_long_double()
    re = np.asarray(re, dtype=np.float64).astype(np.longdouble)
    im = np.asarray(im, dtype=np.float64).astype(np.longdouble)
    re, im = _dft_axes(re, im, -1)
    cells = np.longdouble(re.size)
    return re / cells, im / cells


def _phase_product(shape, at, sign):
    """prod_d exp(-sign 2 pi i k_d at_d / n_d) over the grid, (re, im) long double [nz, ny, nx]:
    one vector of n_d phases per axis, multiplied out."""
    re = np.ones((1, 1, 1), dtype=np.longdouble)
    im = np.zeros((1, 1, 1), dtype=np.longdouble)
    for axis, (n, x0) in enumerate(zip(shape, at)):
        assert 0 <= int(x0) < n
        c, s = unit_roots(n)
        index = (np.arange(n, dtype=np.int64) * int(x0)) % n
        where = [1, 1, 1]
        where[axis] = n
        pr, pi = c[index].reshape(where), (sign * s[index]).reshape(where)
        re, im = re * pr - im * pi, re * pi + im * pr
    return re, im


def delta_spectrum(shape, at, amplitude):
    """The transform of `amplitude` in the cell at = (z0, y0, x0) of a grid of zeros, in closed
    form: A exp(-2 pi i (kx x0 / nx + ky y0 / ny + kz z0 / nz)), (re, im) long double."""
    require_long_double()
    re, im = _phase_product(shape, at, 1)
    return np.longdouble(amplitude) * re, np.longdouble(amplitude) * im


def plane_wave(shape, mode, amplitude):
    """The mirror: the inverse transform of a spectrum that holds (amplitude, 0) in the mode
    (kz0, ky0, kx0) and zeros elsewhere, (A / Ntot) exp(+2 pi i (kx0 x / nx + ...)), (re, im)
    long double."""
    require_long_double()
    re, im = _phase_product(shape, mode, -1)
    scale = np.longdouble(amplitude) / np.longdouble(int(np.prod(shape)))
    return scale * re, scale * im


def signed_modes(n):
    return np.array([k if (k < n // 2 or n == 1) else k - n for k in range(n)], dtype=np.float64)


def mode_q(shape, g):
    """q of every mode, float64 [nz, ny, nx]: mx^2 g[0] + my^2 g[1], then + mz^2 g[2]."""
    nz, ny, nx = shape
    mx, my, mz = signed_modes(nx), signed_modes(ny), signed_modes(nz)
    q = (mx * mx)[None, None, :] * g[0] + (my * my)[None, :, None] * g[1]
    return q + (mz * mz)[:, None, None] * g[2]


def shell_sums(spectrum, g, edges_sq):
    """(modes int64 [n], per bin the list of its p, outside, nonfinite) of a spectrum
    [nz, ny, nx, 2], in the order the definition states."""
    e = np.asarray(edges_sq, dtype=np.float64)
    n = e.size - 1
    p = spectrum[..., 0] * spectrum[..., 0] + spectrum[..., 1] * spectrum[..., 1]
    q = mode_q(spectrum.shape[:3], g)
    finite = np.isfinite(p)
    inside = finite & (e[0] <= q) & (q <= e[n])
    bins = np.minimum(np.searchsorted(e, q, side="right") - 1, n - 1)
    modes = np.bincount(bins[inside], minlength=n).astype(np.int64)
    terms = [p[inside & (bins == b)].tolist() for b in range(n)]
    return modes, terms, int(np.count_nonzero(finite & ~inside)), int(np.count_nonzero(~finite))


def brute_force_modes(dims, cell_size, edges):
    """The counts from a plain loop over the modes with physical wave numbers, square roots and
    all: independent of the squared-edge rule (for edges no mode lies on)."""
    nx, ny, nz = dims
    e = list(edges)
    counts, outside = [0] * (len(e) - 1), 0
    for kz in range(nz):
        for ky in range(ny):
            for kx in range(nx):
                k2 = 0.0
                for k, n, h in ((kx, nx, cell_size[0]), (ky, ny, cell_size[1]),
                                (kz, nz, cell_size[2])):
                    m = k if (k < n // 2 or n == 1) else k - n
                    k2 += (2.0 * math.pi * m / (n * h)) ** 2
                k_abs = math.sqrt(k2)
                if k_abs < e[0] or k_abs > e[-1]:
                    outside += 1
                    continue
                b = max(i for i in range(len(e) - 1) if e[i] <= k_abs)
                counts[b] += 1
    return counts, outside
